"""``HipBackend`` -- the MI355X-native ``AbstractBackend`` for TensorNetwork.

Mirrors ``tensornetwork/backends/abstract_backend.py`` (interface) and
``backends/numpy/numpy_backend.py`` (semantics, error behaviour).  Every method
that touches tensor data lowers to hand-written gfx950 kernels through the C ABI
in ``include/tnh.h``; there is no NumPy/PyTorch compute path in here.  Shape
arithmetic (``shape_*``), argument validation and the SVD truncation rule stay
on the host, exactly as in the reference.
"""
import ctypes
import functools
import io
import numbers

import numpy as np

from tensornetwork_amd import _lib
from tensornetwork_amd.abstract import BackendBase, HAVE_TENSORNETWORK
from tensornetwork_amd import device_tensor
from tensornetwork_amd.device_tensor import (DeviceTensor, bfloat16, public_dtype,
                                             storage_of, tnh_dtype)

_FLOAT_CODES = (_lib.F32, _lib.F64, _lib.BF16, _lib.F16, _lib.C64, _lib.C128)
_INT_CODES = (_lib.I32, _lib.I64)
_NUM_CODES = _FLOAT_CODES + _INT_CODES   # everything the arithmetic kernels take (ints: exact, wrap-around)
_HALF = (_lib.BF16, _lib.F16)
_REAL_OF = {_lib.C64: _lib.F32, _lib.C128: _lib.F64}
_PLAN_CODES = (_lib.BF16, _lib.F16, _lib.F32, _lib.F64, _lib.C64, _lib.C128)     # dtypes whose tensordot lowering is cached


class _TensordotPlan:
  """One lowering of the permute + ONE GEMM path (HipBackend._plan_generic)."""
  __slots__ = ("out_shape", "free_a", "free_b", "trans_a", "trans_b", "m", "n", "k", "lda", "ldb", "code", "out_code",
               "out_bytes", "complex", "native", "perm_a", "perm_b", "k1_a", "k1_b")
# promotion lattice for mixed-dtype binary ops / contractions (numpy's rules,
# with bf16 treated like float16: any mix with a wider float wins).
_RANK = {_lib.BF16: 0, _lib.F16: 0, _lib.F32: 1, _lib.F64: 2, _lib.C64: 3, _lib.C128: 4}


def _vp(t):
  return ctypes.c_void_p(t.ptr)


def _prod(xs):
  out = 1
  for x in xs:
    out *= int(x)
  return out


def _promote(c1, c2):
  if c1 == c2:
    return c1
  i1, i2 = c1 in _INT_CODES, c2 in _INT_CODES
  if i1 and i2:
    return _lib.I64
  if i1 or i2:
    # NumPy: int32 / int64 with a float -> float64, with a complex -> complex128
    other = c2 if i1 else c1
    return _lib.C128 if other in _REAL_OF else _lib.F64
  if {c1, c2} == {_lib.BF16, _lib.F16}:
    return _lib.F32
  hi = c1 if _RANK[c1] >= _RANK[c2] else c2
  lo = c2 if hi == c1 else c1
  if hi == _lib.C64 and lo == _lib.F64:
    return _lib.C128
  return hi


def _np_dtype(t):
  return None if t.dtype is bfloat16 else np.dtype(t.dtype)


def _int_result(*tensors):
  """(code, alias) of an integer-valued result of `tensors` under NumPy's promotion rules, or None when
  an operand is not an integer / bool tensor (the float lattice of _promote applies then)."""
  if not all(t.code in _INT_CODES for t in tensors):
    return None
  return storage_of(np.result_type(*[_np_dtype(t) for t in tensors]))


def _sum_alias(t):
  """NumPy sums unsigned integers in uint64 and bool / signed ones in int64."""
  return np.dtype(np.uint64) if (t.alias is not None and t.alias.kind == "u") else None


def _row_major_strides(shape):
  strides = [1] * len(shape)
  for d in range(len(shape) - 2, -1, -1):
    strides[d] = strides[d + 1] * int(shape[d + 1])
  return strides


def _merge_levels(shape, strides, axes):
  """[(extent, stride)] of `axes` taken in the given order, with memory-adjacent neighbours merged
  and size-1 axes dropped (they address nothing)."""
  levels = []
  for ax in axes:
    n, st = int(shape[ax]), int(strides[ax])
    if n == 1:
      continue
    if levels and levels[-1][1] == st * n:
      levels[-1] = (levels[-1][0] * n, st)
    else:
      levels.append((n, st))
  return levels


def _operand_view(shape, free_axes, k_axes, strides=None):
  """Two-level strided matrix view (tnh_operand_view) of a dense row-major tensor whose rows are
  `free_axes` (output order) and whose contraction index is `k_axes` (K order), or None when the
  tensor cannot be read in place: more than two memory runs on either side, no contiguous
  direction, an inner contraction run that is not a multiple of 32, or misaligned strides."""
  if strides is None:
    strides = _row_major_strides(shape)          # (a row-padded contraction result passes its own)
  rows = _merge_levels(shape, strides, free_axes)
  ks = _merge_levels(shape, strides, k_axes)
  if not ks or len(rows) > 2 or len(ks) > 2:
    return None
  if not rows:
    rows = [(1, 0)]
  r0, sr0 = rows[-1]
  sr1 = rows[0][1] if len(rows) == 2 else 0
  k0, sk0 = ks[-1]
  sk1 = ks[0][1] if len(ks) == 2 else 0
  if (sk0 == 1) == (sr0 == 1):
    return None                      # exactly one contiguous direction
  if k0 % 32 != 0:
    return None
  if sk0 == 1:
    if sr0 % 8 or sr1 % 8 or sk1 % 8:
      return None
  elif sk0 % 8 or sk1 % 8 or sr1 % 8 or r0 % 8:
    return None
  return _lib.OperandView(r0, sr0, sr1, k0, sk0, sk1)


def _gather_descriptor(shape, k_axes, max_box_k=192):
  """see _gather_descriptor_cached: the same few (shape, axes) come back slice after slice"""
  return _gather_descriptor_cached(tuple(int(n) for n in shape), tuple(int(x) for x in k_axes), int(max_box_k))


@functools.lru_cache(maxsize=512)
def _gather_descriptor_cached(shape, k_axes, max_box_k):
  """Tile plan (tnh_gather_desc, include/tnh.h) for reading a dense row-major tensor in place as the long operand
  of tnh_gemm_gather: rows = the free axes in natural order, K = `k_axes` in memory order.  Returns
  (descriptor, BN, long_rows) or None when no box of 64 / 48 free tuples x all contracted indices
  exists whose pieces are 8-byte aligned (the caller then permutes, as before).  More than `max_box_k`
  contracted indices: the box takes the innermost contracted digits that fit and the ONE remaining
  (outermost) contracted digit becomes the K loop (descriptor.kl_ext steps); anything else is None.

  Digits are the tensor's axes innermost first, with size-1 axes dropped and memory-adjacent axes of the same
  role merged.  A box takes the contracted digits in full, the free digits below the split digit in full, and
  T indices of the split digit (T divides its extent); the tile number runs over the rest of the split digit
  and the free digits above it."""
  strides = _row_major_strides(shape)
  kset = set(int(x) for x in k_axes)
  digits = []                                   # [extent, stride, contracted?], innermost first
  for ax in range(len(shape) - 1, -1, -1):
    n = int(shape[ax])
    if n == 1:
      continue
    is_k = ax in kset
    if digits and digits[-1][2] == is_k:
      digits[-1][0] *= n                        # dense row-major: neighbours of one role are one run
    else:
      digits.append([n, int(strides[ax]), is_k])
  free = [i for i, d in enumerate(digits) if not d[2]]
  if not free or len(free) == len(digits) or digits[0][0] % 4:
    return None
  # K loop: contracted digits beyond max_box_k indices (innermost first) -- exactly one may be left over
  kl_ext, kl_stride, box_k = 1, 0, 1
  looped = None
  for i, d in enumerate(digits):
    if not d[2]:
      continue
    if looped is not None:
      return None                               # two contracted digits outside the box
    if box_k * d[0] <= max_box_k:
      box_k *= d[0]
    else:
      looped, kl_ext, kl_stride = i, d[0], d[1]
  if looped is not None:
    if box_k % 8 or box_k < 8 or looped == 0:
      return None
    digits = [d for i, d in enumerate(digits) if i != looped]
    # (removing the digit may leave two free digits as neighbours in the list: they are NOT merged -- their strides
    #  differ by the looped digit's extent -- which the box / tile logic below does not need)
    free = [i for i, d in enumerate(digits) if not d[2]]
  # the split digit: whole free digits while they fit, then T of the next one
  below, split, t_split, bn = 1, None, 0, 0
  for i in free:
    ext = digits[i][0]
    for target in (64, 48):
      if target % below == 0 and ext % (target // below) == 0:
        split, t_split, bn = i, target // below, target
        break
    if split is not None:
      break
    if below * ext >= 48:
      return None
    below *= ext
  if split is None:
    return None
  if split == 0 and t_split % 4:
    return None
  # (the descriptor holds 32-bit offsets inside a box and 64-bit box origins.  Descriptors for the narrow kernels keep
  #  their older rule, the whole tensor below 2^31 elements; the wide kernel's -- bond D = 16 is 2^32 elements -- bound
  #  the box alone, as tnh_gemm_gather itself does)
  if max_box_k <= 192:
    span = sum((d[0] - 1) * d[1] for d in digits)
  else:
    span = sum(((t_split if i == split else d[0]) - 1) * d[1] for i, d in enumerate(digits) if d[2] or i <= split)
  if span >= 1 << 31 or kl_ext > 4096 or (kl_ext > 1 and kl_stride % 4):
    return None
  desc = _lib.GatherDesc()
  nd, w_row, w_k = 0, 1, 1
  for i, (ext, stride, is_k) in enumerate(digits):
    if not is_k and i > split:
      continue
    if nd == _lib.GATHER_MAX_DIGITS:
      return None
    inside = t_split if i == split else ext
    desc.ext[nd], desc.stride[nd] = inside, stride
    if is_k:
      desc.mult[nd] = w_k
      desc.k_mask |= 1 << nd
      w_k *= ext
    else:
      desc.mult[nd] = w_row
      w_row *= inside
    nd += 1
  desc.nd = nd
  nt, rows = 0, bn
  for i in free:
    if i < split:
      continue
    ext, stride = digits[i][0], digits[i][1]
    count, step = (ext // t_split, stride * t_split) if i == split else (ext, stride)
    rows *= count
    if count == 1:
      continue
    if nt == _lib.GATHER_MAX_TILE_DIGITS:
      return None
    desc.text[nt], desc.tstride[nt] = count, step
    nt += 1
  desc.nt = nt
  desc.kl_ext, desc.kl_stride = kl_ext, kl_stride
  return desc, bn, rows


def _scatter_descriptor(shape, k_axes, out_strides, small_ext, small_strides, max_box_k=192):
  """see _scatter_descriptor_cached"""
  return _scatter_descriptor_cached(tuple(int(n) for n in shape), tuple(int(x) for x in k_axes),
                                    tuple(int(s) for s in out_strides), tuple(int(n) for n in small_ext),
                                    tuple(int(s) for s in small_strides), int(max_box_k))


@functools.lru_cache(maxsize=512)
def _scatter_descriptor_cached(shape, k_axes, out_strides, small_ext, small_strides, max_box_k):
  """Output descriptor (tnh_scatter_desc, include/tnh.h) that goes with `_gather_descriptor(shape, k_axes, max_box_k)`
  (192: the narrow kernel's box bound; 256: the wide kernel's, which also bounds the box alone by 2^31 elements) for
  tnh_gemm_gather_scatter: `out_strides[ax]` = elements of the destination per index of the long tensor's axis `ax`
  (contracted axes: anything), `small_ext` / `small_strides` = the small operand's free axes in the order of its rows
  (outermost first) with their destination strides.  Returns (gather descriptor, scatter descriptor, BN, run_elements)
  or None: no one-box gather plan, or a digit of the plan -- memory-adjacent free axes merged into one -- whose indices
  are not evenly spaced in the destination (those axes were pulled apart or swapped there).  `run_elements`: the
  contiguous run of the destination the kernel's stores are made of, 0 when its innermost axis is neither the small
  operand's innermost free axis nor the box's innermost free digit (the kernel refuses those)."""
  plan = _gather_descriptor_cached(shape, k_axes, max_box_k)
  if plan is None or plan[0].kl_ext != 1 or not 1 <= len(small_ext) <= _lib.SCATTER_MAX_SMALL_DIGITS:
    return None
  desc, bn, rows = plan

  def out_step(ext, stride):
    """destination elements per index of a digit (extent, stride in the long tensor), None when not evenly spaced"""
    idx = np.unravel_index(np.arange(ext, dtype=np.int64) * stride, shape)
    off = sum(i.astype(np.int64) * s for i, s in zip(idx, out_strides) if s)
    off = np.broadcast_to(off, (ext,))
    step = int(off[1]) if ext > 1 else 0
    return step if np.array_equal(off, np.arange(ext, dtype=np.int64) * step) else None

  out = _lib.ScatterDesc()
  box = []                                       # free digits of the box: (extent, destination step)
  for d in range(desc.nd):
    if (desc.k_mask >> d) & 1:
      continue
    step = out_step(desc.ext[d], desc.stride[d])
    if step is None:
      return None
    out.omult[d] = step
    box.append((desc.ext[d], step))
  for d in range(desc.nt):
    step = out_step(desc.text[d], desc.tstride[d])
    if step is None:
      return None
    out.otstride[d] = step
  out.ns = len(small_ext)
  for d, (ext, stride) in enumerate(zip(reversed(small_ext), reversed(small_strides))):
    out.sext[d], out.sstride[d] = ext, stride
  out.c_elems = rows * _prod(small_ext)
  run = 0
  for side in (list(zip(reversed(small_ext), reversed(small_strides))), box):
    side = [(e, s) for e, s in side if e != 1]
    if side and side[0][1] == 1:
      run = 1
      for ext, stride in side:
        if stride != run:
          break
        run *= ext
  return desc, out, bn, run


# default of HipBackend.gather_scatter_wide_min_run_bytes ("off": None).  32 bytes, the shortest run there is at D = 16,
# was 1.6-1.9 x faster than wide gather + K1 pass in every call (profiles/gather_scatter_wide.md)
_GATHER_SCATTER_WIDE_MIN_RUN = "32"
_VIEW_SCATTER_MIN_RUN = "24"      # default of HipBackend.view_scatter_min_run_bytes (profiles/view_scatter.md)


def _cview_descriptor(ext_a, ext_b, order, keep_a, keep_b):
  """see _cview_descriptor_cached"""
  return _cview_descriptor_cached(tuple(int(n) for n in ext_a), tuple(int(n) for n in ext_b),
                                  tuple(int(p) for p in order), bool(keep_a), bool(keep_b))


@functools.lru_cache(maxsize=512)
def _cview_descriptor_cached(ext_a, ext_b, order, keep_a, keep_b):
  """Destination descriptor (tnh_cview_desc, include/tnh.h) of tnh_gemm_view_scatter for a product whose operands have
  the free extents `ext_a` / `ext_b` (natural axis order) and whose result is wanted as
  transpose([a's free axes..., b's free axes...], order).  `keep_x`: operand x is read in place, so its rows run over
  its free axes in natural order; an operand that takes a K1 pass anyway is permuted with its free axes in destination
  order, which makes the runs as long as the destination allows.  The operand that owns the destination's innermost
  axis becomes the kernel's N side (`n_is_a`: `a` does, the caller passes `b` as A and `a` as B); that axis must be the
  last of its row axes.  Adjacent digits whose destination strides chain are merged.  Returns (descriptor, n_is_a,
  positions of a's free axes in row order, the same for b, run elements, destination shape) or None: the innermost
  axis is not the last row axis of an operand read in place, more than 6 digits on a side, or a run that is no multiple
  of 4."""
  na = len(ext_a)
  ext = (ext_a, ext_b)
  dest = [(0, p) if p < na else (1, p - na) for p in order]      # destination axis -> (operand, position among its free axes)
  shape = tuple(ext[src][i] for src, i in dest)
  stride_of = dict(zip(dest, _row_major_strides(shape)))
  inner = [d for d in dest if ext[d[0]][d[1]] != 1]
  if not inner:
    return None
  n_src = inner[-1][0]
  used, digits = [], []
  for src, keep in ((0, keep_a), (1, keep_b)):
    rows = list(range(len(ext[src]))) if keep else [i for s, i in dest if s == src]
    merged = []                                  # innermost first: [extent, destination stride]
    for i in reversed(rows):
      e, st = ext[src][i], stride_of[(src, i)]
      if e == 1:
        continue
      if merged and st == merged[-1][0] * merged[-1][1]:
        merged[-1][0] *= e
      else:
        merged.append([e, st])
    if not merged or len(merged) > _lib.CVIEW_MAX_DIGITS:
      return None
    used.append(tuple(rows))
    digits.append(merged)
  run = digits[n_src][0][0]
  if digits[n_src][0][1] != 1 or run % 4:
    return None
  out = _lib.CViewDesc()
  m_side, n_side = digits[1 - n_src], digits[n_src]
  out.nm, out.nn = len(m_side), len(n_side)
  for d, (e, st) in enumerate(m_side):
    out.mext[d], out.mstride[d] = e, st
  for d, (e, st) in enumerate(n_side):
    out.next[d], out.nstride[d] = e, st
  out.run = run
  out.c_elems = _prod(shape)
  return out, n_src == 0, used[0], used[1], run, shape


def _view_scatter_loop(va, m, vb, n, k):
  """Does `tnh_gemm_view_scatter` have a loop for these operand views (A = the M side, rows m; B = the N side, rows n)?
  The host rules of tnh_gemm_bf16.hip, so that nothing is paid for a product the entry then refuses: a K-contiguous A;
  B K-contiguous, or k-major with contraction runs of both operands that are multiples of 64 (the whole-K-tile walk);
  and rows the lean loop can address with 32-bit offsets (`lean_view_rows`)."""
  if va.sk0 != 1:
    return False
  b_km = vb.sk0 != 1
  run_a = k if va.k0 >= k or va.sk1 == va.k0 else va.k0              # (a run that continues seamlessly is one run)
  run_b = k if vb.k0 >= k or vb.sk1 == vb.k0 * vb.sk0 else vb.k0
  if b_km:
    if run_a % 64 or run_b % 64:
      return False
    half_walk = False
  else:
    half_walk = not (run_a == k and run_b == k) and (run_a % 64 != 0 or run_b % 64 != 0)
  lim = 1 << 31                                                      # elements (2 bytes each)

  def rows_ok(v, rows, run, kmajor):
    if v.sr0 <= 0:
      return False
    jump = 64 * v.sk0 if kmajor else (v.sk1 - run if half_walk and run < k else 0)
    if jump < 0 or jump >= lim // 2:
      return False
    r0 = min(v.r0, rows)
    single = r0 >= rows
    inner = (r0 - 1) * v.sr0
    if single or v.sr1 > inner:
      span = (255 * v.sr0 if single else inner + (255 // r0 + 2) * v.sr1) + 64 + jump
      if span < lim:
        return True
    if not single and v.sr1 < 0:
      return False
    whole = ((rows - 1) * v.sr0 if single else inner + ((rows - 1) // r0) * v.sr1) + 64 + jump
    return whole < lim

  return rows_ok(va, m, run_a, False) and rows_ok(vb, n, run_b, b_km)


def _view_tail_split(m, n, k, cus):
  """Would `tnh_gemm_view` cut the last tile rows of this product off into a split-K launch (`+tail_splitk`)?  The rule
  of gemm_bf16_view (tnh_gemm_bf16.hip), which the scattered entry never applies."""
  tiles_m, tiles_n, nkt = (m + 255) // 256, (n + 255) // 256, k // 64
  nwg = tiles_m * tiles_n
  if nwg <= cus or nkt < 96:
    return False
  base = (nwg + cus - 1) // cus
  for rt in range(1, min(32, tiles_m - 1) + 1):
    tail = rt * tiles_n
    s = min(cus // tail, 16)
    if s < 2:
      continue
    ks = (nkt + s - 1) // s
    if ks < 8:
      continue
    s_eff = (nkt + ks - 1) // ks
    cost = ((tiles_m - rt) * tiles_n + cus - 1) // cus + ((tail * s_eff + cus - 1) // cus) * ks / nkt + 0.10
    if cost <= 0.94 * base:
      return True
  return False


def _gather_piece_bytes(desc, itemsize=2):
  """bytes of the contiguous pieces of memory a box is made of (its leading digits while each starts where the
  one before ends)"""
  run = 1
  for d in range(desc.nd):
    if desc.stride[d] != run:
      break
    run *= desc.ext[d]
  return run * itemsize


MAX_KERNEL_RANK = 16      # TNH_MAX_RANK of include/tnh.h: what ONE K1 / K5 launch can index


def _coalesce_permutation(shape, perm):
  """(shape', perm') of the same data movement with fewer axes: extent-1 axes dropped, source axes that stay adjacent
  and in order in the output merged.  `perm[i]` = source axis of output axis i."""
  keep = [p for p in perm if shape[p] != 1]
  if not keep:
    return [1], [0]
  runs = [[keep[0]]]
  for p in keep[1:]:
    if p == runs[-1][-1] + 1 and all(shape[q] == 1 for q in range(runs[-1][-1] + 1, p)):
      runs[-1].append(p)
    else:
      # extent-1 axes between two source axes do not separate them in memory
      last = runs[-1][-1]
      if p > last and all(shape[q] == 1 for q in range(last + 1, p)):
        runs[-1].append(p)
      else:
        runs.append([p])
  order = sorted(range(len(runs)), key=lambda r: runs[r][0])          # the runs in source order
  pos = {r: i for i, r in enumerate(order)}
  cshape = [_prod(shape[a] for a in runs[r]) for r in order]
  return cshape, [pos[r] for r in range(len(runs))]


def _permute_passes(shape, perm, limit=MAX_KERNEL_RANK):
  """A permutation of any rank as a list of (shape_i, perm_i) passes with at most `limit` axes each (after
  coalescing).  One pass whenever the coalesced permutation fits -- always for rank <= 16.  Otherwise every pass moves
  the next (limit - 2) // 2 output axes into place behind the finished prefix: the prefix is one merged axis, the moved
  axes split the rest into at most that many + 1 runs that keep their order, so the pass has <= limit axes."""
  shape, perm = list(shape), list(perm)
  cshape, cperm = _coalesce_permutation(shape, perm)
  if len(cshape) <= limit:
    return [(cshape, cperm)]
  step = (limit - 2) // 2
  order = list(range(len(shape)))            # source axes in their current memory order
  passes, done = [], 0
  while order != perm:
    cur_shape = [shape[a] for a in order]
    direct = [order.index(a) for a in perm]
    cshape, cperm = _coalesce_permutation(cur_shape, direct)
    if len(cshape) <= limit:
      passes.append((cshape, cperm))
      break
    moved = perm[done:done + step]
    new_order = perm[:done + step] + [a for a in order[done:] if a not in moved]
    cshape, cperm = _coalesce_permutation(cur_shape, [order.index(a) for a in new_order])
    assert len(cshape) <= limit, (len(cshape), limit)
    passes.append((cshape, cperm))
    order, done = new_order, done + step
  return passes


def _coalesce_strided(shape, *stride_lists):
  """Merge adjacent axes of a strided iteration space wherever EVERY operand walks them as one run
  (stride[d] == stride[d + 1] * shape[d + 1], zero strides included); extent-1 axes dropped."""
  dims = [d for d in range(len(shape)) if shape[d] != 1]
  if not dims:
    return [1], [[0] for _ in stride_lists]
  oshape, ostr = [shape[dims[0]]], [[st[dims[0]]] for st in stride_lists]
  for d in dims[1:]:
    if all(o[-1] == st[d] * shape[d] for o, st in zip(ostr, stride_lists)):
      oshape[-1] *= shape[d]
      for o, st in zip(ostr, stride_lists):
        o[-1] = st[d]
    else:
      oshape.append(shape[d])
      for o, st in zip(ostr, stride_lists):
        o.append(st[d])
  return oshape, ostr



class HipBackend(BackendBase):
  """TensorNetwork backend running on one MI355X through libtnhip.so.

  Args:
    device: HIP device index for this process (default ``$LOCAL_RANK`` or 0).
    half_output: dtype of bf16/f16 contraction results: ``"same"`` (default,
      what NumPy semantics give) or ``"float32"`` (keep the fp32 accumulator).
    manage_gc: ``True`` opts in to ``gc.freeze()`` at initialisation (cheap full collections in front of
      large allocations); ``False`` keeps the backend's hands off Python's cyclic collector altogether (no
      freeze, no ``gc.collect()`` in front of large allocations); default ``None`` = the policy of
      ``tensornetwork_amd.configure_gc`` / the environment (``TNH_GC_FREEZE``, ``TNH_GC_COLLECT``): no
      freeze, collect only where a measured pass is cheaper than the hipMalloc it avoids.  See DESIGN.md
      section 3 and INTEGRATION.md.
  """

  def __init__(self, device=None, half_output="same", manage_gc=None):
    super().__init__()
    self.name = "hip"
    if half_output not in ("same", "float32"):
      raise ValueError("half_output must be 'same' or 'float32'")
    self.half_output = half_output
    self._device = device
    self._lib = None
    if manage_gc is not None:
      device_tensor.configure_gc(freeze=bool(manage_gc), collect_before_large_alloc=bool(manage_gc))
    # bf16 / f16 tensordot: let the GEMM loaders absorb transposes (tnh_gemm_view) instead of K1 permutes.
    # TNH_ABSORB_TRANSPOSES=0 keeps the permute + NT lowering (A/B and second opinion in the tests).
    import os  # pylint: disable=import-outside-toplevel
    self.absorb_transposes = os.environ.get("TNH_ABSORB_TRANSPOSES", "1") != "0"
    self.pad_results = os.environ.get("TNH_PAD_RESULTS", "0") == "1"       # see _result_pitch
    self.pad_min_bytes = int(os.environ.get("TNH_PAD_MIN_BYTES", str(2 << 30)))
    self.inplace_max_bytes = int(os.environ.get("TNH_VIEW_INPLACE_MAX_BYTES", str(2 << 30)))
    # bf16 / f16 tensordot of a small tensor with a many-axis intermediate: the streaming GEMM gathers the
    # intermediate where it lies (tnh_gemm_gather) instead of K1-permuting it first (TNH_GATHER_GEMM=0: off).
    # Measured per product (profiles/r04_gather_gemm.md): 1.4 - 2.4 x faster than permute + streaming GEMM for
    # every placement of the contracted axes.  Inside a PLANNED path (contractors, ncon) a box made of pieces
    # shorter than `gather_min_piece_bytes` keeps the classic lowering: there the K1 pass also lays the operand
    # out for the contractions that follow (one permute serves two products of the D = 12 network).
    self.gather_gemm = os.environ.get("TNH_GATHER_GEMM", "1") != "0"
    self.gather_min_rows = 1 << 16
    self.gather_min_piece_bytes = int(os.environ.get("TNH_GATHER_MIN_PIECE", "256"))
    # Small operands of 193 ... `gather_max_small` free tuples (bond D = 16: 256) against ONE box of up to 256
    # contracted indices go to the wide kernel (tnh_gemm_gather_wide.hip), but only where the lowerings below would
    # K1-permute the long operand (TNH_GATHER_WIDE=0: 192, the wide kernel is never asked).
    self.gather_max_small = 192 if os.environ.get("TNH_GATHER_WIDE", "1") == "0" else 256
    self.gather_launches = 0     # tnh_gemm_gather launches
    # `tensordot_planned(..., result_order=...)`: the gather GEMM writes its result straight in the axis order the
    # caller names (tnh_gemm_gather_scatter) instead of natural order + one K1 permute (TNH_GATHER_SCATTER=0: off).
    # `gather_scatter_min_run_bytes`: the contiguous run of the destination from which the CONTRACTORS ask for it
    # (None: they do not).  24 bytes, the shortest run there is at D = 12, already beat gather + K1 3.6 x
    # (profiles/gather_scatter.md).
    self.gather_scatter = os.environ.get("TNH_GATHER_SCATTER", "1") != "0"
    _min_run = os.environ.get("TNH_GATHER_SCATTER_MIN_RUN", "24")      # "off": the contractors never ask
    self.gather_scatter_min_run_bytes = int(_min_run) if _min_run.isdigit() else None
    self.gather_scatter_launches = 0     # tnh_gemm_gather_scatter launches
    # The wide form of the same entry (193 ... `gather_max_small` free tuples, tnh_gemm_gather_scatter_wide.hip) takes
    # every explicit `result_order` it can store; `gather_scatter_wide_min_run_bytes` is the run from which
    # `scatter_run_bytes` tells the CONTRACTORS about it (None: it answers 0 for that range) -- see
    # profiles/gather_scatter_wide.md for where the value comes from.
    _min_run = os.environ.get("TNH_GATHER_SCATTER_WIDE_MIN_RUN", _GATHER_SCATTER_WIDE_MIN_RUN)      # "off": never
    self.gather_scatter_wide_min_run_bytes = int(_min_run) if _min_run.isdigit() else None
    # The same for the products of the 256 x 256 view GEMM (tnh_gemm_view_scatter; TNH_VIEW_SCATTER=0: off).
    # `view_scatter_min_run_bytes`: the contiguous run of the destination from which the backend takes the scattered
    # form at all (None: never) -- see profiles/view_scatter.md for where the value comes from.
    self.view_scatter = os.environ.get("TNH_VIEW_SCATTER", "1") != "0"
    _min_run = os.environ.get("TNH_VIEW_SCATTER_MIN_RUN", _VIEW_SCATTER_MIN_RUN)      # "off": never
    self.view_scatter_min_run_bytes = int(_min_run) if _min_run.isdigit() else None
    self.view_scatter_launches = 0       # tnh_gemm_view_scatter launches
    # A product whose last, mostly empty wave of tiles `tnh_gemm_view` would split over K (`_view_tail_split`: the rule
    # of gemm_bf16_view) keeps the usual lowering, because the scattered entry never splits: 20736 x 1728 x 20736 ran
    # 1.33 ms scattered against 1.09-1.14 ms for tail split + K1 pass (profiles/view_scatter.md).
    # TNH_VIEW_SCATTER_KEEP_TAIL_SPLIT=0: scatter those too.
    self.view_scatter_keep_tail_split = os.environ.get("TNH_VIEW_SCATTER_KEEP_TAIL_SPLIT", "1") != "0"
    self._cus = None
    # The contractors (`contract_between`, `ncon`, `contract_path`) put their question to `scatter_run_bytes` only while
    # `gather_scatter_min_run_bytes` is set, and compare the answer with it: TNH_GATHER_SCATTER_MIN_RUN=off keeps them
    # from asking for these products too, and a `view_scatter_min_run_bytes` below it takes effect only for direct
    # callers of `tensordot_planned(..., result_order=...)`.
    self.permutes_absorbed = 0   # tnh_gemm_view launches
    self.permute_launches = 0    # K1 launches (transpose)
    self._direct_launches = type(self).transpose is HipBackend.transpose and type(self)._gemm is HipBackend._gemm
    self._td_plans = {}          # tensordot: lowering plans of the permute + ONE GEMM path by (shapes, axes, dtype, hints)
    self.gemm_events = None      # bench.py: a list that receives (start, stop) HIP events around every GEMM launch
    self._svd_band_failed = set()      # per backend object (the class attributes below only say what they are)
    self._svd_band_backoff = {}

  # the backend is a per-process singleton bound to one device: copies are the object itself
  def __copy__(self):
    return self

  def __deepcopy__(self, memo):
    return self

  def __reduce__(self):
    return (get_hip_backend, ())

  # ------------------------------------------------------------------ plumbing
  @property
  def lib(self):
    if self._lib is None:
      self._lib = _lib.init(self._device)
      device_tensor.freeze_collector_baseline()
    return self._lib

  def synchronize(self):
    _lib.check(self.lib.tnh_sync(), "tnh_sync")

  def _check_float(self, t, what):
    if t.code not in _FLOAT_CODES:
      raise NotImplementedError(f"{what} is not implemented for dtype {t.dtype} on the hip backend")

  def _check_num(self, t, what):
    # int32 / int64 run the same contraction / reduction / arithmetic kernels exactly (the reference
    # hands any NumPy dtype to np.tensordot / np.sum / np.trace: numpy_backend.py:35-54, 603-607, 684-707)
    if t.code not in _NUM_CODES:
      raise NotImplementedError(f"{what} is not implemented for dtype {t.dtype} on the hip backend")

  def _as_tensor(self, x):
    if isinstance(x, DeviceTensor):
      return self._dense(x)
    return self.convert_to_tensor(x)

  def _dense(self, tensor):
    """The dense row-major copy of a row-padded contraction result (DeviceTensor.pad; only produced when
    `pad_results` is on), any other tensor as it is.  Every entry point except the in-place contraction lowering
    works on dense tensors."""
    if tensor.pad is None:
      return tensor
    split, pitch = tensor.pad
    rows, row = _prod(tensor.shape[:split]), _prod(tensor.shape[split:])
    out = DeviceTensor.empty(tensor.shape, tensor.code, tensor.alias)
    if tensor.size:
      _lib.check(self.lib.tnh_strided_copy(_vp(out), _vp(tensor), 2, _lib.i64_array((rows, row)),
                                           _lib.i64_array((pitch, 1)), 0, tensor.itemsize), "tnh_strided_copy")
    return out

  def _result_pitch(self, m, n, itemsize):
    """Row pitch (elements) of an m x n contraction result: n, or n + 64 when `pad_results` is on and the rows are
    a power of two of 2 KiB or more in a result of `pad_min_bytes` or more.  Why: a later contraction that re-views
    such a result with rows of 1 MiB or more finds ALL its rows at the same offset modulo the pitch -- the same few
    HBM channels -- and runs at 850 TFLOP/s whatever the data (profiles/r03_gemm_epilogue.md section 5: 1.05-1.65
    PFLOP/s with 128 bytes of padding per row).  Off by default until it has been measured on the workload it is for
    (the chi = 32 MERA layer): TNH_PAD_RESULTS=1 or `be.pad_results = True`."""
    row_bytes = n * itemsize
    if not self.pad_results or row_bytes < 2048 or row_bytes & (row_bytes - 1) or m * row_bytes < self.pad_min_bytes:
      return n
    return n + 64

  def _canonical(self, tensor, alias=None):
    """A bool / unsigned / narrow-integer tensor is stored widened to int64 and stays exact under +, -, * only
    modulo 2^bits; everything else -- conversion to another dtype, sums, division, abs, sign -- must see the value
    NumPy holds in the narrow type: wrapped (zero- or sign-extended low bits), bool as 0 / 1 (tnh_wrap_int)."""
    alias = tensor.alias if alias is None else alias
    if alias is None or tensor.code != _lib.I64 or not tensor.size:
      return tensor
    mode = 2 if alias.kind == "b" else (0 if alias.kind == "u" else 1)
    if mode != 2 and alias.itemsize == 8:
      return tensor
    out = DeviceTensor.empty(tensor.shape, _lib.I64, tensor.alias)
    _lib.check(self.lib.tnh_wrap_int(_vp(out), _vp(tensor), tensor.size, 8 * alias.itemsize, mode), "tnh_wrap_int")
    return out

  def cast(self, tensor, dtype):
    """Device-side dtype conversion (bf16/f16/f32/f64, real->complex)."""
    code, alias = (dtype, None) if isinstance(dtype, int) else storage_of(dtype)
    if tensor.code == code:
      if tensor.alias == alias:
        return tensor
      # another narrow type on the same int64 storage: the source's canonical value, then (to bool) != 0
      t = self._canonical(tensor)
      t = DeviceTensor(t._block, t.shape, code, t._offset, alias)   # pylint: disable=protected-access
      return self._canonical(t) if alias is not None and alias.kind == "b" else t
    self._check_num(tensor, "cast")
    tensor = self._canonical(self._dense(tensor))
    if alias is not None and alias.kind == "b" and tensor.code not in _INT_CODES:
      # float -> bool is (x != 0), not a truncation (0.5 is True): sign(x)^2 is exactly 0 or 1
      if tensor.is_complex:
        tensor = self._unary(_lib.OP_ABS, tensor)
      sgn = self._unary(_lib.OP_SIGN, tensor)
      tensor = self._binary(_lib.OP_MUL, sgn, sgn)
    if tensor.is_complex and code not in _REAL_OF:
      raise TypeError(f"cannot cast {tensor.dtype} to a real dtype: the imaginary part would be discarded")
    out = DeviceTensor.empty(tensor.shape, code, alias)
    _lib.check(self.lib.tnh_cast(_vp(out), code, _vp(tensor), tensor.code, tensor.size), "tnh_cast")
    return out

  # -------------------------------------------------------------------- ingest
  def convert_to_tensor(self, tensor):
    # numpy_backend.py:92-97: ndarray or scalar, else TypeError.
    if isinstance(tensor, DeviceTensor):
      return tensor
    if not isinstance(tensor, np.ndarray) and not np.isscalar(tensor):
      raise TypeError("Expected a `np.array` or scalar. Got {}".format(type(tensor)))
    self.lib  # pylint: disable=pointless-statement
    return DeviceTensor.from_numpy(np.asarray(tensor))

  def to_bfloat16(self, array):
    """Host array -> bf16 tensor in HBM (round-to-nearest-even on the host)."""
    self.lib  # pylint: disable=pointless-statement
    if isinstance(array, DeviceTensor):
      return self.cast(array, _lib.BF16)
    return DeviceTensor.from_numpy(np.asarray(array), dtype=bfloat16)

  # ------------------------------------------------------------ shape helpers
  def shape_concat(self, values, axis):
    return np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for v in values], axis)

  def shape_tensor(self, tensor):
    return tensor.shape

  def shape_tuple(self, tensor):
    return tensor.shape

  def sparse_shape(self, tensor):
    return self.shape_tuple(tensor)

  def shape_prod(self, values):
    return np.prod(values)

  # ------------------------------------------------------------------- layout
  def reshape(self, tensor, shape):
    padded = tensor if isinstance(tensor, DeviceTensor) and tensor.pad is not None else None
    tensor = self._as_tensor(tensor) if padded is None else tensor
    shape = [int(s) for s in np.asarray(shape).astype(np.int64).reshape(-1)]
    neg = [i for i, s in enumerate(shape) if s == -1]
    if len(neg) > 1:
      raise ValueError("can only specify one unknown dimension")
    if neg:
      known = _prod(s for s in shape if s != -1)
      if known == 0 or tensor.size % known:
        raise ValueError(f"cannot reshape array of size {tensor.size} into shape {tuple(shape)}")
      shape[neg[0]] = tensor.size // known
    if _prod(shape) != tensor.size:
      raise ValueError(f"cannot reshape array of size {tensor.size} into shape {tuple(shape)}")
    if padded is not None:
      # a row-padded contraction result (pad_results): reshape is on the contractors' path (flatten_edges), so the
      # padding is kept whenever the new shape keeps the row boundary -- only then densified
      try:
        return padded.view(shape)
      except ValueError:
        tensor = self._dense(padded)
    return tensor.view(shape)

  def transpose(self, tensor, perm=None):
    tensor = self._as_tensor(tensor)
    nd = tensor.ndim
    if perm is None:
      perm = tuple(range(nd - 1, -1, -1))
    perm = tuple(int(p) + nd if int(p) < 0 else int(p) for p in perm)
    if sorted(perm) != list(range(nd)):
      raise ValueError("axes don't match array")
    if perm == tuple(range(nd)):
      return tensor
    out_shape = [tensor.shape[p] for p in perm]
    if nd > MAX_KERNEL_RANK:
      # more axes than one K1 launch indexes: coalesce (axes that travel together are one axis to the kernel); a
      # permutation that still has more than 16 independent runs takes several passes (_permute_passes)
      cur = tensor
      for cshape, cperm in _permute_passes(tensor.shape, perm):
        if cperm == list(range(len(cperm))):
          continue
        nxt = DeviceTensor.empty([cshape[p] for p in cperm], tensor.code, tensor.alias)
        self.permute_launches += 1
        _lib.check(self.lib.tnh_permute(_vp(nxt), _vp(cur), len(cshape), _lib.i64_array(cshape),
                                        _lib.i32_array(cperm), tensor.itemsize), "tnh_permute")
        cur = nxt
      return cur.view(out_shape) if cur is not tensor else self.copy(tensor).view(out_shape)
    out = DeviceTensor.empty(out_shape, tensor.code, tensor.alias)
    self.permute_launches += 1
    _lib.check(self.lib.tnh_permute(_vp(out), _vp(tensor), nd, _lib.i64_array(tensor.shape),
                                    _lib.i32_array(perm), tensor.itemsize), "tnh_permute")
    return out

  def _strided_copy(self, tensor, shape, strides, offset):
    out = DeviceTensor.empty(shape, tensor.code, tensor.alias)
    kshape, kstrides = list(shape), list(strides)
    if len(kshape) > MAX_KERNEL_RANK:
      kshape, (kstrides,) = _coalesce_strided(kshape, kstrides)
      if len(kshape) > MAX_KERNEL_RANK:
        raise NotImplementedError(f"a strided window with {len(kshape)} independent axes (one launch indexes "
                                  f"{MAX_KERNEL_RANK}): slice it in two steps")
    _lib.check(self.lib.tnh_strided_copy(_vp(out), _vp(tensor), len(kshape), _lib.i64_array(kshape),
                                         _lib.i64_array(kstrides), int(offset), tensor.itemsize),
               "tnh_strided_copy")
    return out

  def slice_into(self, out, tensor, start_indices):
    """out[...] = tensor[start : start + out.shape] written into the EXISTING block of `out`
    (one strided gather, no allocation): refreshes the fixed input buffers of a captured
    hipGraph (see ``capture``)."""
    tensor = self._as_tensor(tensor)
    if len(start_indices) != tensor.ndim or out.ndim != tensor.ndim or out.code != tensor.code:
      raise ValueError("slice_into: rank / dtype mismatch")
    st = _row_major_strides(tensor.shape)
    for s0, n, dim in zip(start_indices, out.shape, tensor.shape):
      if s0 < 0 or s0 + n > dim:
        raise ValueError("slice_into: window out of range")
    offset = sum(int(s0) * int(t) for s0, t in zip(start_indices, st))
    _lib.check(self.lib.tnh_strided_copy(_vp(out), _vp(tensor), out.ndim, _lib.i64_array(out.shape),
                                         _lib.i64_array(st), int(offset), tensor.itemsize),
               "tnh_strided_copy")
    return out

  def capture(self, fun, *args):
    """Record every kernel launch of ``fun(*args)`` into a hipGraph instead of running it.

    The MI355X-native stand-in for ``jit`` on launch-bound contraction sequences (many small
    pairwise steps): ``g = backend.capture(f, *tensors)``, then ``g.launch()`` replays the
    whole sequence with one submission and returns the same output tensors (same HBM
    blocks) every time.  Inputs are read at their captured addresses: refresh them in
    place (``slice_into`` / ``copy_into``) between launches.  ``fun`` must not read
    results back to the host (no ``item``/``numpy``/``svd`` inside)."""
    return DeviceGraph(self, fun, args)

  def copy(self, tensor):
    """A new block holding the same data (device to device)."""
    tensor = self._as_tensor(tensor)
    out = DeviceTensor.empty(tensor.shape, tensor.code, tensor.alias)
    if tensor.nbytes:
      _lib.check(self.lib.tnh_d2d(_vp(out), _vp(tensor), tensor.nbytes), "tnh_d2d")
    return out

  def copy_into(self, out, tensor):
    tensor = self._as_tensor(tensor)
    if out.nbytes != tensor.nbytes or out.code != tensor.code:
      raise ValueError("copy_into: size / dtype mismatch")
    _lib.check(self.lib.tnh_d2d(_vp(out), _vp(tensor), out.nbytes), "tnh_d2d")
    return out

  def copy_rows_into(self, out, tensor, row0):
    """out[row0 : row0 + tensor.shape[0]] = tensor (leading-axis block copy, device to device)."""
    tensor = self._as_tensor(tensor)
    if out.code != tensor.code or tuple(out.shape[1:]) != tuple(tensor.shape[1:]) or \
        row0 < 0 or row0 + tensor.shape[0] > out.shape[0]:
      raise ValueError("copy_rows_into: block does not fit")
    row_bytes = _prod(out.shape[1:]) * out.itemsize
    _lib.check(self.lib.tnh_d2d(ctypes.c_void_p(out.ptr + row0 * row_bytes), _vp(tensor), tensor.nbytes), "tnh_d2d")
    return out

  def concat_rows(self, tensors):
    """Concatenate along the leading axis (device-to-device block copies)."""
    tensors = [self._as_tensor(t) for t in tensors]
    out = DeviceTensor.empty((sum(t.shape[0] for t in tensors),) + tuple(tensors[0].shape[1:]), tensors[0].code,
                             tensors[0].alias)
    row = 0
    for t in tensors:
      self.copy_rows_into(out, t, row)
      row += t.shape[0]
    return out

  def slice(self, tensor, start_indices, slice_sizes):
    # numpy_backend.py:64-72
    if len(start_indices) != len(slice_sizes):
      raise ValueError("Lengths of start_indices and slice_sizes must be"
                       "identical.")
    tensor = self._as_tensor(tensor)
    key = tuple(slice(int(s), int(s) + int(n)) for s, n in zip(start_indices, slice_sizes))
    return self.getitem(tensor, key)

  def getitem(self, tensor, key):
    """Basic (int / slice / Ellipsis) indexing, materialised by one gather."""
    tensor = self._dense(tensor)
    if not isinstance(key, tuple):
      key = (key,)
    if any(k is Ellipsis for k in key):
      i = [n for n, k in enumerate(key) if k is Ellipsis][0]
      fill = tensor.ndim - (len(key) - 1)
      key = key[:i] + (slice(None),) * fill + key[i + 1:]
    if len(key) > tensor.ndim:
      raise IndexError("too many indices for tensor")
    key = key + (slice(None),) * (tensor.ndim - len(key))
    in_strides = _row_major_strides(tensor.shape)
    shape, strides, offset = [], [], 0
    for dim, k, st in zip(tensor.shape, key, in_strides):
      if isinstance(k, slice):
        start, stop, step = k.indices(dim)
        n = len(range(start, stop, step))
        shape.append(n)
        strides.append(st * step)
        offset += start * st
      elif isinstance(k, numbers.Integral):
        k = int(k)
        if k < -dim or k >= dim:
          raise IndexError(f"index {k} is out of bounds for axis with size {dim}")
        offset += (k % dim) * st
      else:
        raise NotImplementedError("hip backend supports int/slice indexing only")
    return self._strided_copy(tensor, shape, strides, offset)

  # -------------------------------------------------------------- contraction
  def _gemm(self, a, b, trans_a, trans_b, m, n, k, lda, ldb, batch=1, stride_a=0, stride_b=0,
            out_shape=None, out_code=None, alias=None):
    code = a.code
    if out_code is None:
      out_code = _lib.F32 if (code in _HALF and self.half_output == "float32") else code
    out = DeviceTensor.empty(out_shape if out_shape is not None else (m, n), out_code, alias)
    events = getattr(self, "gemm_events", None)
    if events is not None:  # bench.py: HIP events on the launch stream around the GEMM only
      start = _lib.Event().record()
    _lib.check(self.lib.tnh_gemm(code, out_code, int(trans_a), int(trans_b), m, n, k, _vp(a), lda,
                                 _vp(b), ldb, _vp(out), n, batch, stride_a, stride_b, m * n), "tnh_gemm")
    if events is not None:
      events.append((start, _lib.Event().record()))
    return out

  @staticmethod
  def _normalize_axes(a, b, axes):
    """numpy.tensordot's axes argument -> two equal-length lists of ints."""
    try:
      iter(axes)
    except TypeError:
      n = int(axes)
      if n < 0:
        raise ValueError("axes must be non-negative")  # pylint: disable=raise-missing-from
      axes_a = list(range(a.ndim - n, a.ndim))
      axes_b = list(range(0, n))
    else:
      axes_a, axes_b = axes
      try:
        axes_a = [int(x) for x in axes_a]
      except TypeError:
        axes_a = [int(axes_a)]
      try:
        axes_b = [int(x) for x in axes_b]
      except TypeError:
        axes_b = [int(axes_b)]
    if len(axes_a) != len(axes_b):
      raise ValueError("shape-mismatch for sum")
    axes_a = [x + a.ndim if x < 0 else x for x in axes_a]
    axes_b = [x + b.ndim if x < 0 else x for x in axes_b]
    for x, y in zip(axes_a, axes_b):
      if not (0 <= x < a.ndim and 0 <= y < b.ndim) or a.shape[x] != b.shape[y]:
        raise ValueError("shape-mismatch for sum")
    if len(set(axes_a)) != len(axes_a) or len(set(axes_b)) != len(axes_b):
      raise ValueError("repeated axis in tensordot")
    return axes_a, axes_b

  def tensordot(self, a, b, axes):
    return self._tensordot_impl(a, b, axes, None, None)[0]

  def tensordot_planned(self, a, b, axes, free_order_a=None, free_order_b=None, allow_swap=False, result_order=None):
    """``tensordot`` whose result may carry the free axes of an operand in a caller-chosen order
    -- but only where that is FREE: an operand that needs a K1 permute anyway (its contracted axes
    are neither leading nor trailing) is permuted straight into ``free_order_x + contracted``;
    an operand consumed in place keeps its natural order.  Returns ``(tensor, used_a, used_b)``
    with the free axes of ``a`` / ``b`` in result order.  The contractors use it to lay a big
    intermediate out for the NEXT contractions while they pay for the current permute
    (tensornetwork_amd.contractors.contract_path): permutes are HBM-bound, skipping one saves
    2 x bytes of traffic.

    ``allow_swap=True`` (callers for whom the axis order of the result is bookkeeping) returns a fourth value
    ``swapped``: when true the result carries ``b``'s free axes FIRST, then ``a``'s -- the gather lowering writes
    [long operand's axes..., small operand's axes] whichever operand the long one is, because that output tile is
    one contiguous block of memory.

    ``result_order`` (a permutation of the result's axes, expressed over ``[a's free axes..., b's free axes...]`` in
    their natural order) fixes the axis order of the result outright: the tensor comes back as
    ``transpose(tensordot(a, b, axes), result_order)``, bit for bit.  Where the gather GEMM takes the product it
    writes that order itself (``tnh_gemm_gather_scatter``, no K1 pass over the result); everywhere else the usual
    lowering runs, followed by one ``transpose``.  The per-operand orders and ``allow_swap`` are not consulted then;
    ``used_a`` / ``used_b`` are the natural free axes and ``swapped`` is false."""
    if result_order is not None:
      out = self._tensordot_ordered(a, b, axes, result_order)
      return out if allow_swap else out[:3]
    out = self._tensordot_impl(a, b, axes, free_order_a, free_order_b, allow_swap)
    return out if allow_swap else out[:3]

  def _tensordot_ordered(self, a, b, axes, result_order):
    """`tensordot_planned` with `result_order`: (tensor in that order, natural free_a, natural free_b, False)"""
    a = a if isinstance(a, DeviceTensor) else self.convert_to_tensor(a)
    b = b if isinstance(b, DeviceTensor) else self.convert_to_tensor(b)
    axes_a, axes_b = self._normalize_axes(a, b, axes)
    free_a = [i for i in range(a.ndim) if i not in axes_a]
    free_b = [i for i in range(b.ndim) if i not in axes_b]
    order = [int(p) for p in result_order]
    if sorted(order) != list(range(len(free_a) + len(free_b))):
      raise ValueError(f"result_order {result_order} is not a permutation of the result's {len(free_a) + len(free_b)} axes")
    if order == list(range(len(order))):      # natural order: nothing to scatter, the usual lowering as it is
      return self._tensordot_impl(a, b, (axes_a, axes_b), None, None)[0], free_a, free_b, False
    got = None
    if a.code == b.code and a.code in _HALF and self.gather_gemm and self.gather_scatter and \
        self.half_output == "same" and axes_a:
      got = self._tensordot_gather_scatter(a, b, axes_a, axes_b, free_a, free_b, order)
    if got is None and axes_a:
      got = self._tensordot_view_scatter(a, b, axes_a, axes_b, free_a, free_b, order)
    if got is None:
      got = self.transpose(self._tensordot_impl(a, b, (axes_a, axes_b), None, None)[0], order)
    return got, free_a, free_b, False

  def scatter_run_bytes(self, a, b, axes, result_order):
    """Bytes of the contiguous runs `tnh_gemm_gather_scatter` would store for this product and order, 0 where the
    product is not one the scatter lowering takes (nothing is launched).  The contractors compare it with
    `gather_scatter_min_run_bytes`.  As this is the question of a PLANNED path, `_tensordot_gather`'s rule for those
    holds here too: a box made of pieces shorter than `gather_min_piece_bytes` keeps the classic lowering, whose K1 pass
    also lays the long operand out for later products.  A small operand at an address the kernel would refuse (a sliced
    view that is not 16-byte aligned) gives 0 as well, so that the contractors never pay the fallback's transpose to an
    interleaved order.  (A variant forced through `tnh_gemm_set_variant`, an A/B and test knob, is not visible here:
    with one set, an order asked for on the strength of this answer costs the usual lowering + one K1 pass.)
    For a product of the 256 x 256 view GEMM the answer is the run `tnh_gemm_view_scatter` would store, under
    `_view_scatter_plan`'s rules (0 below `view_scatter_min_run_bytes`, for tail-split products and for operand forms
    the entry has no loop for)."""
    if not (isinstance(a, DeviceTensor) and isinstance(b, DeviceTensor) and a.code == b.code and a.code in _HALF and
            self.half_output == "same"):
      return 0
    axes_a, axes_b = self._normalize_axes(a, b, axes)
    if not axes_a:
      return 0
    free_a = [i for i in range(a.ndim) if i not in axes_a]
    free_b = [i for i in range(b.ndim) if i not in axes_b]
    order = [int(p) for p in result_order]
    # the products of the view GEMM (tnh_gemm_view_scatter): the run, from `view_scatter_min_run_bytes` on
    vplan = self._view_scatter_plan(a, b, axes_a, axes_b, free_a, free_b, order)
    if vplan is not None:
      return vplan[0][4] * a.itemsize
    if not (self.gather_gemm and self.gather_scatter and getattr(self.lib, "tnh_gemm_gather_scatter", None) is not None):
      return 0
    plan = self._scatter_plan(a, b, axes_a, axes_b, free_a, free_b, order)
    if plan is None or _gather_piece_bytes(plan[0][0], a.itemsize) < self.gather_min_piece_bytes:
      return 0
    small = a if plan[1] else b
    if small.ptr % 16:
      return 0
    run_bytes = plan[0][3] * a.itemsize
    if min(_prod(a.shape[i] for i in free_a), _prod(b.shape[i] for i in free_b)) > 192:
      # the wide form has a threshold of its own (None: the contractors never ask for it)
      wide_min = self.gather_scatter_wide_min_run_bytes
      if wide_min is None or run_bytes < wide_min:
        return 0
    return run_bytes

  def _scatter_plan(self, a, b, axes_a, axes_b, free_a, free_b, order):
    """The descriptors of `_tensordot_gather_scatter` for this product: ((gather descriptor, scatter descriptor, BN,
    run elements), small_first, small operand's free axes in destination order, destination shape), or None."""
    m = _prod(a.shape[i] for i in free_a)
    n = _prod(b.shape[i] for i in free_b)
    k = _prod(a.shape[i] for i in axes_a)
    small_first = m <= n
    ms, nl = (m, n) if small_first else (n, m)
    # 193 ... `gather_max_small` free tuples: the wide form (tnh_gemm_gather_scatter_wide.hip), one box of up to 256
    wide = 192 < ms <= self.gather_max_small
    if not ((wide and 8 <= k <= 256) or (64 < ms <= 192 and 16 <= k <= 192)) or k % 8 or nl < self.gather_min_rows:
      return None
    long_ = b if small_first else a
    small = a if small_first else b
    if long_.pad is not None or long_.ptr % 8:
      return None
    # destination axis p = natural result axis order[p]: an axis of a (source 0) or of b (source 1)
    natural = [(0, i) for i in free_a] + [(1, i) for i in free_b]
    dest = [natural[p] for p in order]
    shape = tuple((a, b)[src].shape[i] for src, i in dest)
    strides = _row_major_strides(shape)
    long_src = 1 if small_first else 0
    out_strides = [0] * long_.ndim
    used_s, small_strides = [], []
    for (src, i), st in zip(dest, strides):
      if src == long_src:
        out_strides[i] = st
      else:
        used_s.append(i)
        small_strides.append(st)
    axes_l = axes_b if small_first else axes_a
    plan = _scatter_descriptor(long_.shape, axes_l, out_strides, [small.shape[i] for i in used_s], small_strides,
                               256 if wide else 192)
    if plan is None or plan[3] == 0 or plan[3] % 4:      # (run 0: an innermost axis the kernel does not store along)
      return None
    return plan, small_first, used_s, shape

  def _tensordot_gather_scatter(self, a, b, axes_a, axes_b, free_a, free_b, order):
    """One `tnh_gemm_gather_scatter` launch: the product `_tensordot_gather` takes (a small operand of 65 ... 192 free
    tuples, or 193 ... `gather_max_small` through the wide form, against ONE box of a long tensor read where it lies; here
    also with trailing contracted axes), written in
    the axis order `order` over [free_a..., free_b...].  Only the small operand is permuted, to [its free axes in the
    order they have in the destination, contracted axes in the long tensor's memory order].  Or None (nothing
    launched): the caller runs the usual lowering and one transpose; results are bit-identical either way."""
    launch = getattr(self.lib, "tnh_gemm_gather_scatter", None)
    if launch is None:
      return None
    plan = self._scatter_plan(a, b, axes_a, axes_b, free_a, free_b, order)
    if plan is None:
      return None
    (desc, out_desc, _, _), small_first, used_s, shape = plan
    small, long_ = (a, b) if small_first else (b, a)
    axes_s, axes_l = (axes_a, axes_b) if small_first else (axes_b, axes_a)
    by_memory = sorted(range(len(axes_l)), key=lambda i: axes_l[i])
    small = self.transpose(self._dense(small), used_s + [axes_s[i] for i in by_memory])
    if small.ptr % 16:
      return None
    ms, k = _prod(small.shape[:len(used_s)]), _prod(small.shape[len(used_s):])
    out = DeviceTensor.empty(shape, long_.code)
    events = getattr(self, "gemm_events", None)
    if events is not None:
      start = _lib.Event().record()
    status = launch(long_.code, ms, k, out.size // ms, _vp(small), k, _vp(long_), long_.size, ctypes.byref(desc),
                    _vp(out), ctypes.byref(out_desc))
    if status == _lib.ERR_UNSUPPORTED:
      return None     # (a forced A/B variant, TNH_GATHER_SCATTER=0, or an alignment rule: nothing was launched)
    _lib.check(status, "tnh_gemm_gather_scatter")
    if events is not None:
      events.append((start, _lib.Event().record()))
    self.gather_scatter_launches += 1
    return out

  def _view_scatter_plan(self, a, b, axes_a, axes_b, free_a, free_b, order):
    """What `_tensordot_view_scatter` would do for this product and order, nothing launched: (`_cview_descriptor`'s
    values, (a, its view, its K1 pass or None), the same for b) with the operand choice of `_view_choice`, or None --
    the form is off, the product is not the view GEMM's (or one a gather lowering may take, or one whose tail the view
    GEMM would split over K), the destination is one the kernel does not store, its run is below
    `view_scatter_min_run_bytes`, or the operand views are ones the entry has no loop for.  Host arithmetic only; on
    the contractors' path it runs twice per product (`scatter_run_bytes`, then the lowering): tensors are not kept
    alive in a cache for it."""
    if not (self.view_scatter and self.view_scatter_min_run_bytes is not None and self.absorb_transposes and
            a.code == b.code and a.code in _HALF and self.half_output == "same" and
            getattr(self.lib, "tnh_gemm_view_scatter", None) is not None):
      return None
    m = _prod(a.shape[i] for i in free_a)
    n = _prod(b.shape[i] for i in free_b)
    k = _prod(a.shape[i] for i in axes_a)
    if min(m, n) <= self.gather_max_small or (self.view_scatter_keep_tail_split and
                                              _view_tail_split(m, n, k, self._compute_units())):
      return None
    choice = self._view_choice(a, b, axes_a, axes_b, free_a, free_b, m, n, k)
    if choice is None:
      return None
    ka, kb, va, vb = choice
    plan = _cview_descriptor([a.shape[i] for i in free_a], [b.shape[i] for i in free_b], order, va is not None,
                             vb is not None)
    if plan is None or plan[4] * a.itemsize < self.view_scatter_min_run_bytes:
      return None
    # the K1 pass of an operand that is not read in place: (tensor, permutation, view of the result), not run yet
    pass_a = pass_b = None
    if va is None:
      pass_a = self._k_blocked_plan(a, [free_a[i] for i in plan[2]], ka, m, k)
      va = pass_a[2]
    if vb is None:
      pass_b = self._k_blocked_plan(b, [free_b[i] for i in plan[3]], kb, n, k)
      vb = pass_b[2]
    # what the entry would refuse (a k-major operand on the M side, a k-major N side without the whole-K-tile walk,
    # rows the lean loop cannot address) is refused here, before a pass is paid or a contractor asks for the order
    if not (_view_scatter_loop(vb, n, va, m, k) if plan[1] else _view_scatter_loop(va, m, vb, n, k)):
      return None
    return plan, (a, va, pass_a), (b, vb, pass_b)

  def _compute_units(self):
    """CUs of the device (what the view GEMM's tail split is sized by)"""
    if self._cus is None:
      cus, hbm = ctypes.c_int(0), ctypes.c_int64(0)
      info = getattr(self.lib, "tnh_device_info", None)
      ok = info is not None and info(ctypes.create_string_buffer(64), 64, ctypes.byref(cus), ctypes.byref(hbm)) == 0
      self._cus = cus.value if ok and cus.value > 0 else 256
    return self._cus

  def _tensordot_view_scatter(self, a, b, axes_a, axes_b, free_a, free_b, order):
    """One `tnh_gemm_view_scatter` launch: the product `_tensordot_in_place` takes, with the same operands read in
    place, written in the axis order `order` over [free_a..., free_b...] by the GEMM's own epilogue.  The operand that
    owns the destination's innermost axis is the kernel's N side (`b` is passed as A and `a` as B when it is `a`); an
    operand that takes a K1 pass anyway is permuted to [its free axes in destination order, contracted axes].  Or None
    (no GEMM launched): the caller runs the usual lowering and one transpose; results are bit-identical either way."""
    plan = self._view_scatter_plan(a, b, axes_a, axes_b, free_a, free_b, order)
    if plan is None:
      return None
    (desc, n_is_a, _, _, _, shape), (a, va, pass_a), (b, vb, pass_b) = plan
    m = _prod(a.shape[i] for i in free_a)
    n = _prod(b.shape[i] for i in free_b)
    k = _prod(a.shape[i] for i in axes_a)
    if pass_a is not None:
      a = self.transpose(pass_a[0], pass_a[1])
    if pass_b is not None:
      b = self.transpose(pass_b[0], pass_b[1])
    out = DeviceTensor.empty(shape, a.code)
    if n_is_a:
      a, va, m, b, vb, n = b, vb, n, a, va, m
    events = getattr(self, "gemm_events", None)
    if events is not None:
      start = _lib.Event().record()
    status = self.lib.tnh_gemm_view_scatter(a.code, m, n, k, _vp(a), ctypes.byref(va), _vp(b), ctypes.byref(vb),
                                            _vp(out), ctypes.byref(desc))
    if status == _lib.ERR_UNSUPPORTED:
      return None     # (a forced A/B variant or knob: the plan has already refused what the entry's own rules refuse)
    _lib.check(status, "tnh_gemm_view_scatter")
    if events is not None:
      events.append((start, _lib.Event().record()))
    self.view_scatter_launches += 1
    return out

  def _tensordot_impl(self, a, b, axes, hint_a, hint_b, allow_swap=False):
    """c[free_a..., free_b...] = sum_axes a*b (abstract_backend.py:27-38).

    Lowered as transpose + reshape + ONE GEMM (the reference's own spec for this
    is backends/tensorflow/tensordot2.py:22-250): an operand is used in place
    when its contracted axes are already leading or trailing (the GEMM absorbs
    the transpose through its row/column strides); otherwise one K1 permute
    brings it to [free, contracted] form.  For bf16/f16 both operands are
    brought to the K-contiguous form the 16x16x32 MFMA kernels consume.
    """
    # Fast lane (round 6): small products are host-bound (a D = 32 `contract_between` spent 23 us of Python in this
    # function for ~5 us of kernels), and a contraction path calls with the same (shapes, axes, dtype, hints) over and
    # over: the lowering of the permute + ONE GEMM path is a pure function of those, planned once (`_plan_generic`)
    # and replayed (`_run_plan`: ctypes arrays made once, no axis arithmetic).  Products the gather / in-place
    # lowerings may take are never planned here: those look at addresses and policy.
    key = None
    if self.plan_cache and type(a) is DeviceTensor and type(b) is DeviceTensor and a._code == b._code and \
        a._code in _PLAN_CODES and a._pad is None and b._pad is None and self.gemm_events is None:   # pylint: disable=protected-access
      try:
        key = (a._shape, b._shape, tuple(axes[0]), tuple(axes[1]), a._code,     # pylint: disable=protected-access
               None if hint_a is None else tuple(hint_a), None if hint_b is None else tuple(hint_b), allow_swap,
               self.gather_gemm, self.absorb_transposes, self.half_output, self.gather_max_small, self.complex_lowering)
        plan = self._td_plans.get(key)
      except TypeError:      # (an integer `axes`, unhashable entries: the general walk below)
        key = plan = None
      if plan is not None:
        return self._run_plan(plan, a, b, None)
    a = a if isinstance(a, DeviceTensor) else self.convert_to_tensor(a)     # (row-padded results stay as they lie
    b = b if isinstance(b, DeviceTensor) else self.convert_to_tensor(b)     #  until the in-place lowering has looked)
    axes_a, axes_b = self._normalize_axes(a, b, axes)
    ires = _int_result(a, b)
    code, alias = ires if ires is not None else (_promote(a.code, b.code), None)
    a, b = self.cast(a, code), self.cast(b, code)
    self._check_num(a, "tensordot")

    free_a = [i for i in range(a.ndim) if i not in axes_a]
    free_b = [i for i in range(b.ndim) if i not in axes_b]
    m = _prod(a.shape[i] for i in free_a)
    n = _prod(b.shape[i] for i in free_b)
    k = _prod(a.shape[i] for i in axes_a)
    nc = len(axes_a)
    if nc == 0:
      out_shape = tuple(a.shape[i] for i in free_a) + tuple(b.shape[i] for i in free_b)
      return self._outer(self._dense(a), self._dense(b), out_shape, alias), free_a, free_b, False

    # bf16 / f16, enough 256 x 256 tiles: read BOTH operands in place through two-level strides
    # (K8 lowering of tensordot2.py:62-88 -- transposes are absorbed by the GEMM loaders, no K1 launch).
    if code in _HALF:       # products the gather / in-place lowerings may take (by shape alone) are not planned
      ms, nl = (m, n) if m <= n else (n, m)
      if (64 < ms <= 192 and 16 <= k <= 192 * 4096 and k % 8 == 0 and nl >= self.gather_min_rows) or \
          (192 < ms <= self.gather_max_small and 8 <= k <= 256 and k % 8 == 0 and nl >= self.gather_min_rows) or \
          not (m < 256 or n < 256 or ((m + 255) // 256) * ((n + 255) // 256) < 192 or k % 64 or k < 128):
        key = None

    def gathered(got):
      out, used_a, used_b, swapped = got
      shape_a, shape_b = tuple(a.shape[i] for i in used_a), tuple(b.shape[i] for i in used_b)
      return out.view(shape_b + shape_a if swapped else shape_a + shape_b), used_a, used_b, swapped

    wide = None       # the wide gather kernel's attempt: made where a lowering below is about to permute the long operand
    if code in _HALF and self.gather_gemm and self.half_output == "same":
      got = self._tensordot_gather(a, b, axes_a, axes_b, free_a, free_b, m, n, k, hint_a, hint_b, allow_swap)
      if got is not None:
        return gathered(got)
      if 192 < min(m, n) <= self.gather_max_small:
        tried = []

        def wide():
          if not tried:
            tried.append(self._tensordot_gather(a, b, axes_a, axes_b, free_a, free_b, m, n, k, hint_a, hint_b,
                                                allow_swap, wide=True))
          return tried[0]
    if code in _HALF and self.absorb_transposes:
      a_shape0, b_shape0 = a.shape, b.shape
      got = self._tensordot_in_place(a, b, axes_a, axes_b, free_a, free_b, m, n, k, hint_a, hint_b, wide)
      if got is not None and len(got) == 4:
        return gathered(got)
      if got is not None:
        out, used_a, used_b = got
        out_shape = tuple(a_shape0[i] for i in used_a) + tuple(b_shape0[i] for i in used_b)
        return out.view(out_shape), used_a, used_b, False
    if wide is not None:      # (the permute + ONE GEMM lowering below permutes a long operand whose contracted axes are not trailing)
      got = wide()
      if got is not None:
        return gathered(got)
    a, b = self._dense(a), self._dense(b)
    plan = self._plan_generic(a.shape, b.shape, axes_a, axes_b, free_a, free_b, m, n, k, code, hint_a, hint_b)
    if key is not None and alias is None:
      if len(self._td_plans) >= 4096:
        self._td_plans.clear()
      self._td_plans[key] = plan
    return self._run_plan(plan, a, b, alias)

  def _plan_generic(self, a_shape, b_shape, axes_a, axes_b, free_a, free_b, m, n, k, code, hint_a, hint_b):
    """The permute + ONE GEMM lowering of tensordot as data: which operands get a K1 permute (and where to), the
    storage forms handed to tnh_gemm, the result's shape and the order of the free axes in it.  A pure function of
    its arguments and of `half_output` / `complex_lowering` (parts of the plan cache's key)."""
    if self.complex_lowering not in ("embedded", "native"):
      raise ValueError(f"complex_lowering must be 'embedded' or 'native', got {self.complex_lowering!r}")
    nc = len(axes_a)
    nd_a, nd_b = len(a_shape), len(b_shape)
    # memory order of the contracted pairs on each side
    order_a = sorted(range(nc), key=lambda i: axes_a[i])
    order_b = sorted(range(nc), key=lambda i: axes_b[i])
    sa, sb = sorted(axes_a), sorted(axes_b)
    a_form = "MK" if sa == list(range(nd_a - nc, nd_a)) else (
        "KM" if sa == list(range(nc)) else None)
    b_form = "NK" if sb == list(range(nd_b - nc, nd_b)) else (
        "KN" if sb == list(range(nc)) else None)
    if nd_a == nc:
      a_form = "MK"  # M == 1: both readings are valid, prefer K-contiguous
    if nd_b == nc:
      b_form = "NK"

    # bf16 / f16: the matrix-core kernels (LDS-DMA for aligned shapes, register-staged
    # for ragged ones) take both operands K-contiguous ("NT"); any other storage form is
    # brought there by one K1 permute.  Products too small to care stay in place.
    half_nt = code in _HALF and 2 * m * n * k >= (1 << 18)
    want_a = a_form if (a_form and not (half_nt and a_form != "MK")) else None
    want_b = b_form if (b_form and not (half_nt and b_form != "NK")) else None

    if want_a and want_b and order_a != order_b:
      # contracted axes are paired in a different memory order on the two sides:
      # re-order the smaller operand.
      if _prod(a_shape) <= _prod(b_shape):
        want_a = None
      else:
        want_b = None
    if want_a and not want_b:
      pair_order = order_a
    elif want_b and not want_a:
      pair_order = order_b
    else:
      pair_order = order_a
    free_a, free_b = list(free_a), list(free_b)
    perm_a = perm_b = None
    if not want_a:
      if hint_a is not None and sorted(hint_a) == free_a:
        free_a = [int(i) for i in hint_a]       # the permute is paid anyway: any free order is free
      perm_a = tuple(free_a + [axes_a[i] for i in pair_order])
      a_form = "MK"
      if perm_a == tuple(range(nd_a)):
        perm_a = None
    if not want_b:
      if hint_b is not None and sorted(hint_b) == free_b:
        free_b = [int(i) for i in hint_b]
      perm_b = tuple(free_b + [axes_b[i] for i in pair_order])
      b_form = "NK"
      if perm_b == tuple(range(nd_b)):
        perm_b = None
    plan = _TensordotPlan()
    plan.out_shape = tuple(a_shape[i] for i in free_a) + tuple(b_shape[i] for i in free_b)
    plan.free_a, plan.free_b = tuple(free_a), tuple(free_b)
    plan.trans_a = int(a_form == "KM")
    plan.trans_b = int(b_form == "NK")
    plan.m, plan.n, plan.k = m, n, k
    plan.lda = m if plan.trans_a else k
    plan.ldb = k if plan.trans_b else n
    plan.code = code
    plan.out_code = _lib.F32 if (code in _HALF and self.half_output == "float32") else code
    plan.out_bytes = m * n * device_tensor._ITEMSIZE[plan.out_code]      # pylint: disable=protected-access
    plan.complex = code in _REAL_OF and 8 * m * n * k >= (1 << 18)
    plan.native = plan.complex and self.complex_lowering == "native"
    plan.perm_a, plan.perm_b = perm_a, perm_b
    plan.k1_a = self._plan_permute(a_shape, perm_a, code)
    plan.k1_b = self._plan_permute(b_shape, perm_b, code)
    return plan

  @staticmethod
  def _plan_permute(shape, perm, code):
    """(result shape, its bytes, rank, ctypes shape, ctypes perm, item size) of ONE K1 launch, or None (no permute,
    or more axes than one launch indexes: `transpose` walks those)."""
    if perm is None or len(shape) > MAX_KERNEL_RANK:
      return None
    out_shape = tuple(shape[p] for p in perm)
    item = device_tensor._ITEMSIZE[code]      # pylint: disable=protected-access
    return (out_shape, _prod(out_shape) * item, len(shape), _lib.i64_array(shape), _lib.i32_array(perm), item)

  def _run_plan(self, plan, a, b, alias):
    """Launches of a planned tensordot: at most two K1 permutes and ONE GEMM.  Returns what `_tensordot_impl` does."""
    if not self._direct_launches:      # a subclass hooks `transpose` / `_gemm` (the host dry-run tools): go through them
      if plan.perm_a is not None:
        a = self.transpose(a, plan.perm_a)
      if plan.perm_b is not None:
        b = self.transpose(b, plan.perm_b)
      if plan.complex and not plan.native:
        out = self._complex_gemm(a, b, bool(plan.trans_a), bool(plan.trans_b), plan.m, plan.n, plan.k)
      else:
        out = self._gemm(a, b, bool(plan.trans_a), bool(plan.trans_b), plan.m, plan.n, plan.k, plan.lda, plan.ldb, alias=alias)
      return out.view(plan.out_shape), list(plan.free_a), list(plan.free_b), False
    lib = self.lib
    if plan.perm_a is not None:
      k1 = plan.k1_a
      if k1 is None:
        a = self.transpose(a, plan.perm_a)
      else:
        t = DeviceTensor._fresh(k1[0], plan.code, k1[1], a._alias)      # pylint: disable=protected-access
        self.permute_launches += 1
        _lib.check(lib.tnh_permute(_vp(t), _vp(a), k1[2], k1[3], k1[4], k1[5]), "tnh_permute")
        a = t
    if plan.perm_b is not None:
      k1 = plan.k1_b
      if k1 is None:
        b = self.transpose(b, plan.perm_b)
      else:
        t = DeviceTensor._fresh(k1[0], plan.code, k1[1], b._alias)      # pylint: disable=protected-access
        self.permute_launches += 1
        _lib.check(lib.tnh_permute(_vp(t), _vp(b), k1[2], k1[3], k1[4], k1[5]), "tnh_permute")
        b = t
    m, n, k = plan.m, plan.n, plan.k
    if plan.complex and not plan.native:     # (native: the ONE tnh_gemm below, on the complex operands where they lie)
      out = self._complex_gemm(a, b, bool(plan.trans_a), bool(plan.trans_b), m, n, k).view(plan.out_shape)
      return out, list(plan.free_a), list(plan.free_b), False
    out = DeviceTensor._fresh(plan.out_shape, plan.out_code, plan.out_bytes,      # pylint: disable=protected-access
                              alias if plan.out_code == _lib.I64 else None)
    events = self.gemm_events
    if events is not None:  # bench.py: HIP events on the launch stream around the GEMM only
      start = _lib.Event().record()
    _lib.check(lib.tnh_gemm(plan.code, plan.out_code, plan.trans_a, plan.trans_b, m, n, k, _vp(a), plan.lda,
                            _vp(b), plan.ldb, _vp(out), n, 1, 0, 0, m * n), "tnh_gemm")
    if events is not None:
      events.append((start, _lib.Event().record()))
    return out, list(plan.free_a), list(plan.free_b), False

  def _tensordot_gather(self, a, b, axes_a, axes_b, free_a, free_b, m, n, k, hint_a=None, hint_b=None,
                        allow_swap=False, wide=False):
    """One `tnh_gemm_gather` launch for a SMALL operand (65 ... 192 free tuples) against a long many-axis
    tensor whose contracted axes are not trailing; `wide`: the same for 193 ... `gather_max_small` free tuples and
    at most 256 contracted indices in ONE box (the wide kernel; asked only where the long operand would be permuted
    otherwise).  Or None (the caller's permute + GEMM lowering runs;
    results are bit-identical either way for K <= 192; beyond that the kernel walks the outermost contracted
    axis step by step -- same products, another grouping of the fp32 sums than the tile kernels').  The long tensor is read where it lies, so its free axes
    come out in natural order whatever the planner hinted -- the NEXT contraction gathers it again instead
    of finding it laid out; only the small operand is permuted (to [free, contracted in the long tensor's
    memory order]).  With `allow_swap` the result is [long operand's axes..., small operand's axes] whichever
    operand the long one is: an output tile is then one contiguous block of 14 - 18 KB instead of Ms row
    segments of 96 / 128 bytes (measured: profiles/r04_gather_gemm.md).
    Returns (tensor, used_free_a, used_free_b, swapped)."""
    small_first = m <= n
    ms, nl = (m, n) if small_first else (n, m)
    if wide:
      if not (192 < ms <= self.gather_max_small and 8 <= k <= 256 and k % 8 == 0 and nl >= self.gather_min_rows):
        return None
    elif not (64 < ms <= 192 and 16 <= k <= 192 * 4096 and k % 8 == 0 and nl >= self.gather_min_rows):
      return None
    long_rows_first = not small_first or (allow_swap and ms % 8 == 0)     # C[Nl, Ms]: the kernel's "swap" form
    if long_rows_first and ms % 8:
      return None
    small, long_ = (a, b) if small_first else (b, a)
    axes_s, axes_l = (axes_a, axes_b) if small_first else (axes_b, axes_a)
    free_s, free_l = (free_a, free_b) if small_first else (free_b, free_a)
    hint_s = hint_a if small_first else hint_b
    if long_.pad is not None or long_.ptr % 8:
      return None
    nc = len(axes_l)
    if sorted(axes_l) == list(range(long_.ndim - nc, long_.ndim)):
      return None       # contracted axes trailing: the streaming kernel reads it as it is
    plan = _gather_descriptor(long_.shape, axes_l, max_box_k=256) if wide else _gather_descriptor(long_.shape, axes_l)
    if plan is None:
      return None
    desc, _, rows = plan
    if wide and desc.kl_ext != 1:
      return None
    if desc.kl_ext > 1 and ms * (k // desc.kl_ext // 8) > 11 * 256:
      return None       # (the K-loop kernel re-stages an Ms x K / steps slice of the small operand per step)
    planned = allow_swap or hint_a is not None or hint_b is not None
    if rows != nl or (planned and _gather_piece_bytes(desc, long_.itemsize) < self.gather_min_piece_bytes):
      return None
    order = sorted(range(nc), key=lambda i: axes_l[i])       # the long tensor's memory order of the contracted pairs
    used_s = list(free_s)
    if hint_s is not None and sorted(hint_s) == sorted(free_s):
      used_s = [int(i) for i in hint_s]
    small = self.transpose(self._dense(small), used_s + [axes_s[i] for i in order])
    if small.ptr % 16:
      return None
    out = DeviceTensor.empty((nl, ms) if long_rows_first else (ms, nl), long_.code)
    events = getattr(self, "gemm_events", None)
    if events is not None:
      start = _lib.Event().record()
    status = self.lib.tnh_gemm_gather(long_.code, ms, k, nl, _vp(small), k, _vp(long_), long_.size,
                                      ctypes.byref(desc), _vp(out), ms if long_rows_first else nl,
                                      0 if long_rows_first else 1)
    if status == _lib.ERR_UNSUPPORTED:
      return None     # (a forced A/B variant, TNH_GATHER_GEMM=0, or an alignment rule: nothing was launched)
    _lib.check(status, "tnh_gemm_gather")
    if events is not None:
      events.append((start, _lib.Event().record()))
    self.gather_launches += 1
    used_l = sorted(free_l)
    if small_first:
      return out, used_s, used_l, long_rows_first       # (swapped: b's axes, the long operand's, come first)
    return out, used_l, used_s, False

  def _tensordot_in_place(self, a, b, axes_a, axes_b, free_a, free_b, m, n, k, hint_a=None, hint_b=None, wide=None):
    """One `tnh_gemm_view` launch that reads the operands as they lie in HBM wherever that pays, or None
    (caller falls back to the classic permute + tnh_gemm lowering; results are bit-identical either way).

    The contraction order K is free as long as both sides agree: a's memory order of the contracted axes
    and b's are both tried, and the one that leaves the fewest bytes to permute wins.  An operand is read
    in place when `_operand_view` offers a view and the size / intensity gate in `usable` below lets it.
    Operands that are not read
    in place are permuted to [free..., contracted...] (free order = the planner's hint when given) and
    viewed trivially.  Returns (tensor, used_free_a, used_free_b).  `wide` (the caller's attempt at the wide gather
    kernel, or None) is called where the long operand is about to be permuted; when it delivers, its four values
    (`_tensordot_gather`'s) are returned instead."""
    choice = self._view_choice(a, b, axes_a, axes_b, free_a, free_b, m, n, k, hint_a, hint_b)
    if choice is None:
      return None
    ka, kb, va, vb = choice
    if wide is not None and (vb if m <= n else va) is None:
      # about to K1-permute the long operand: the wide gather kernel reads it where it lies instead (its result is
      # returned as `_tensordot_gather` gives it, four values)
      got = wide()
      if got is not None:
        return got
    used_a, used_b = list(free_a), list(free_b)
    if va is None:
      if hint_a is not None and sorted(hint_a) == sorted(free_a):
        used_a = [int(i) for i in hint_a]
      a, va = self._k_blocked(a, used_a, ka, m, k)
    if vb is None:
      if hint_b is not None and sorted(hint_b) == sorted(free_b):
        used_b = [int(i) for i in hint_b]
      b, vb = self._k_blocked(b, used_b, kb, n, k)
    out_code = _lib.F32 if self.half_output == "float32" else a.code
    ldc = self._result_pitch(m, n, 4 if out_code == _lib.F32 else 2)
    if ldc == n:
      out = DeviceTensor.empty((m, n), out_code)
    else:
      out = DeviceTensor.empty((m * ldc,), out_code).as_rows(m, n, ldc)
    events = getattr(self, "gemm_events", None)
    if events is not None:
      start = _lib.Event().record()
    status = self.lib.tnh_gemm_view(a.code, out_code, m, n, k, _vp(a), ctypes.byref(va), _vp(b), ctypes.byref(vb),
                                    _vp(out), ldc)
    if status == _lib.ERR_UNSUPPORTED:
      return None     # (a forced A/B variant, or an alignment rule: nothing was launched)
    _lib.check(status, "tnh_gemm_view")
    if events is not None:
      events.append((start, _lib.Event().record()))
    self.permutes_absorbed += 1
    return out, used_a, used_b

  def _view_choice(self, a, b, axes_a, axes_b, free_a, free_b, m, n, k, hint_a=None, hint_b=None):
    """The operand choice of the view GEMM lowerings (`_tensordot_in_place`, `_tensordot_view_scatter`): nothing is
    launched.  Returns (ka, kb, va, vb) -- the contracted axes of a / b in the chosen K order and the view of each
    operand that is read in place (None: it takes a K1 pass) -- or None when the product is not the view GEMM's."""
    if m < 256 or n < 256 or ((m + 255) // 256) * ((n + 255) // 256) < 192 or k % 64 or k < 128:
      return None
    if a.ptr % 16 or b.ptr % 16:
      return None     # (a sliced view at an odd offset: tnh_gemm_view would refuse it AFTER the permutes below were paid)
    nc = len(axes_a)
    orders = [sorted(range(nc), key=lambda i: axes_a[i]), sorted(range(nc), key=lambda i: axes_b[i])]
    if orders[0] == orders[1]:
      orders = orders[:1]

    out_bytes = m * n * a.itemsize

    def rows_of(t, free):
      return _prod(t.shape[i] for i in free)

    def usable(t, free, kax, hint, kt_partner=False):
      v = _operand_view(t.shape, free, kax, t.strides if t.pad is not None else None)
      # The planner asked for another order of this operand's free axes (it lays the RESULT out for the contractions
      # that follow) and the operand is small against the result: pay its K1 pass now rather than a pass over the
      # result later (MERA chi = 32: with the runs-of-32 views every small operand became readable in place, and the
      # 68 GB intermediate then needed a 137 GB permute in front of the next product).
      if v is not None and hint is not None and sorted(hint) == sorted(free) and \
          [int(i) for i in hint] != list(free) and 8 * t.nbytes <= out_bytes:
        return None
      # Gate (measured, profiles/r02_lowering_ab.txt): a view of a tensor above `inplace_max_bytes` is given up for
      # ONE K1 pass into a K-contiguous copy when it is k-major (a workgroup streaming it touches 64 new pages per
      # K-tile: -4 ... -10 % GEMM rate), or when it has two-level strides AND the product is so compute-heavy that
      # the copy is free (> 2e4 flop per operand byte: config-2 L1 at D = 256 runs 5 % slower on the strided `a`
      # than on its 3.7 ms copy).  Everything else is read in place: the MERA layer at chi = 32 loses 35 % when
      # its 68 GB intermediates (30 - 1000 flop per byte) are permuted.
      # Round 5 (profiles/r05_kmajor_gate_small.jsonl, r05_kmajor_gate.jsonl): with the lean loops a k-major operand
      # read in place costs the GEMM ~10 % (D = 96 / 128 L0: 1264-1271 / 1336-1356 TFLOP/s in place, 1323-1336 /
      # 1419-1421 through ONE K1 pass; D = 192 / 256 / the D = 512 row: 1233-1245 / 1176 / 1264-1283 against 1400 /
      # 1384-1394 / 1353-1360); only where the pass would cost more than that (D = 64: a 0.1 ms product, 1299-1307
      # against 1201-1203) does the in-place read win.  Estimate: 10 % of the product at 1.45 PFLOP/s against
      # 2 x bytes at 5 TB/s + 6 us.
      # Round 6 (profiles/r06_kmajor_lean_loop.md): a k-major `b` whose contraction runs are multiples of 64, next to a
      # K-contiguous `a`, is read by the interleaved whole-K-tile loop (B_KT in tnh_gemm_bf16.hip: 8 instructions per
      # K-tile more than the NT loop instead of 94).  Its cost is the operand's size, not the loop: nothing up to ~0.6 GB
      # (D = 96 / 128 L0 in place 1379 / 1542 TFLOP/s against 1351 / 1494-1516 through the pass), 2 % at 1 GB, 7 % at
      # 2.7 GB, 10 % at 4.3 GB (B's lines miss the XCD's L2 2.4 times as often as the K-contiguous form's once the
      # contraction is thousands of K-tiles long).
      if v is not None and v.sk0 != 1 and self.kmajor_inplace_penalty > 0.0:
        penalty = self.kmajor_inplace_penalty
        # (measured on consecutive k rows one row pitch apart; config-2 L1 at D = 128 -- k rows 4 MiB apart, 256 bytes of
        #  each -- ran 1384 TFLOP/s in place against ~1435 through the pass: such views keep the round-5 rule)
        if kt_partner and v.k0 % 64 == 0 and self.kmajor_tile_walk and v.sk0 <= self.kmajor_tile_walk_max_pitch:
          penalty = min(penalty, max(0.0, self.kmajor_tile_walk_penalty_per_gb * (t.nbytes / 1e9 - 0.6)))
        if penalty * (2.0 * m * n * k / self.model_gemm_flops) > \
            2.0 * t.nbytes / self.model_k1_bytes_per_s + self.model_launch_s:
          return None
      # Round 6 (profiles/r06_k_blocked_operands.md): a K-contiguous operand whose rows lie a multiple of 1 MiB apart
      # (K = 2^19 and up in bf16) runs the kernel at 1294 TFLOP/s (1 MiB) / 766-789 (2 MiB) instead of ~1500 -- the
      # 256 rows of a tile alias in the memory system, zeros and random data alike.  Where one K1 pass into the
      # K-blocked form (`_k_blocked` below) costs less than that, the view is given up for it.
      if v is not None and v.sk0 == 1 and self.k_blocked_permutes and min(v.r0, rows_of(t, free)) >= 64 and \
          (v.sr0 * t.itemsize) % (1 << 20) == 0:
        loss = 0.15 if v.sr0 * t.itemsize == (1 << 20) else 0.45
        if loss * (2.0 * m * n * k / self.model_gemm_flops) > 2.0 * t.nbytes / self.model_k1_bytes_per_s + self.model_launch_s:
          return None
      if v is not None and t.nbytes > self.inplace_max_bytes:
        plain = v.sk0 == 1 and v.sr1 == 0 and v.sk1 == 0
        # (round 5: a K-contiguous two-level view whose inner contraction run is a multiple of 64 walks K tile by tile in
        #  the lean loop; measured on config-2 L1 (profiles/r05_l1_gate.jsonl): D = 192 (2.7 GB) in place 1467-1477
        #  TFLOP/s with ONE K1 launch against 1451 with two; D = 256 (8.6 GB, power-of-two strides) in place 1314-1319
        #  against 1477 -- so only up to `inplace_strided_max_bytes`)
        tile_walk = v.sk0 == 1 and v.k0 % 64 == 0 and self.inplace_strided_big and t.nbytes <= self.inplace_strided_max_bytes
        if v.sk0 != 1 or (not plain and not tile_walk and 2.0 * m * n * k > 2e4 * t.nbytes):
          return None
      return v

    best = None
    for order in orders:
      ka, kb = [axes_a[i] for i in order], [axes_b[i] for i in order]
      va = usable(a, free_a, ka, hint_a)
      # (`a` permuted = one K-contiguous run; `a` in place: K-contiguous with runs that are multiples of 64)
      vb = usable(b, free_b, kb, hint_b, kt_partner=(va is None and k % 64 == 0) or (va is not None and va.sk0 == 1 and va.k0 % 64 == 0))
      cost = (a.nbytes if va is None else 0) + (b.nbytes if vb is None else 0)
      if best is None or cost < best[0]:
        best = (cost, ka, kb, va, vb)
    return best[1:]

  def _k_blocked(self, t, free, kax, rows, k):
    """The K1 pass that brings an operand of the view GEMM to K-contiguous form, and the view of its result.  Normally
    [free..., contracted...]: rows of k elements.  When such a row would be 1 MiB or longer the result is laid out
    K-BLOCKED instead -- [outer contracted axes..., free..., inner contracted axes...], i.e. rows `inner` elements
    apart and contraction runs of `inner` -- which costs the pass nothing and keeps the 256 rows of a tile out of each
    other's way (the binary-MERA layer at chi = 32, 1024 x 32768 x 2^20: 1088 -> 1493 TFLOP/s; 8192 x 8192 x 2^20:
    766 -> 1480; x 2^19: 1294 -> 1532; profiles/r06_k_blocked_operands.md).  The inner run is the shortest suffix
    of the contracted axes that is a multiple of 64 and at least 512 long (a single long contracted axis is split by
    a reshape first: metadata only)."""
    t, perm, view = self._k_blocked_plan(t, free, kax, rows, k)
    return self.transpose(t, perm), view

  def _k_blocked_plan(self, t, free, kax, rows, k):
    """`_k_blocked` without the pass: (the tensor, re-viewed where an axis is split; the permutation; the view of the
    pass's result)."""
    if self.k_blocked_permutes and k * t.itemsize >= self.k_blocked_min_row_bytes and rows >= 64:
      shape = list(t.shape)
      free, kax = list(free), list(kax)
      if len(kax) == 1 or _prod(shape[i] for i in kax[1:]) < 512:
        # split the first contracted axis: [.., K0, ..] -> [.., K0 / q, q, ..] with q * (the later contracted axes) >= 512
        ax, rest = kax[0], _prod(shape[i] for i in kax[1:])
        q = 1
        while q * rest < 512 and shape[ax] % (2 * q) == 0:
          q *= 2
        if 1 < q < shape[ax] and (q * rest) % 64 == 0 and t.pad is None:
          t = t.view(shape[:ax] + [shape[ax] // q, q] + shape[ax + 1:])
          shape = list(t.shape)
          bump = lambda i: i + 1 if i > ax else i
          free = [bump(i) for i in free]
          kax = [ax, ax + 1] + [bump(i) for i in kax[1:]]
      inner = 1
      for s in range(len(kax) - 1, 0, -1):
        inner *= shape[kax[s]]
        if inner % 64 == 0 and inner >= 512:
          return t, kax[:s] + free + kax[s:], _lib.OperandView(rows, inner, 0, inner, 1, rows * inner)
    return t, list(free) + list(kax), _lib.OperandView(rows, k, 0, k, 1, 0)

  def _complex_gemm(self, a, b, trans_a, trans_b, m, n, k):
    """complex64 / complex128 product on the f32 / f64 matrix cores: the interleaved (re, im)
    memory of a row-major A (M x K) and of C (M x N) are real M x 2K / M x 2N matrices, and
    C_r = A_r B' with B' the 2x2-block real expansion of B (tnh_complex_expand) -- one extra
    pass over B, then ONE real GEMM with the 8 M N K flops a complex GEMM needs."""
    code = a.code
    real = _REAL_OF[code]
    if trans_a:   # A must be row-major M x K for the zero-copy real image
      a = self.transpose(a.view((k, m)), (1, 0))
    bexp = DeviceTensor.empty((2 * k, 2 * n), real)
    rs, cs = (1, k) if trans_b else (n, 1)
    _lib.check(self.lib.tnh_complex_expand(_vp(bexp), _vp(b), k, n, rs, cs, 0, code), "tnh_complex_expand")
    out = DeviceTensor.empty((m, n), code)
    events = getattr(self, "gemm_events", None)
    if events is not None:
      start = _lib.Event().record()
    _lib.check(self.lib.tnh_gemm(real, real, 0, 0, m, 2 * n, 2 * k, _vp(a), 2 * k, _vp(bexp), 2 * n,
                                 _vp(out), 2 * n, 1, 0, 0, 0), "tnh_gemm")
    if events is not None:
      events.append((start, _lib.Event().record()))
    return out

  def _outer(self, a, b, out_shape, alias=None):
    m, n = a.size, b.size
    out = DeviceTensor.empty((m, n), a.code, alias)
    _lib.check(self.lib.tnh_binary(_lib.OP_MUL, _vp(out), _vp(a), _vp(b), 2, _lib.i64_array((m, n)),
                                   _lib.i64_array((1, 0)), _lib.i64_array((0, 1)), a.code), "tnh_binary")
    return out.view(out_shape)

  def outer_product(self, tensor1, tensor2):
    # numpy_backend.py:99-100: np.tensordot(a, b, 0)
    return self.tensordot(tensor1, tensor2, 0)

  def matmul(self, tensor1, tensor2):
    tensor1 = self._as_tensor(tensor1)
    tensor2 = self._as_tensor(tensor2)
    if (tensor1.ndim <= 1) or (tensor2.ndim <= 1):
      raise ValueError("inputs to `matmul` have to be a tensors of order > 1,")
    ires = _int_result(tensor1, tensor2)
    code, alias = ires if ires is not None else (_promote(tensor1.code, tensor2.code), None)
    a, b = self.cast(tensor1, code), self.cast(tensor2, code)
    self._check_num(a, "matmul")
    m, k = a.shape[-2:]
    k2, n = b.shape[-2:]
    if k != k2:
      raise ValueError(f"matmul: Input operand 1 has a mismatch in its core dimension 0 "
                       f"(size {k2} is different from {k})")
    ba, bb = a.shape[:-2], b.shape[:-2]
    if ba == bb:
      batch_shape, stride_a, stride_b = ba, m * k, k * n
    elif not bb:
      batch_shape, stride_a, stride_b = ba, m * k, 0
    elif not ba:
      batch_shape, stride_a, stride_b = bb, 0, k * n
    else:
      batch_shape = tuple(np.broadcast_shapes(ba, bb))
      a = self._broadcast_to(a, batch_shape + (m, k))
      b = self._broadcast_to(b, batch_shape + (k, n))
      stride_a, stride_b = m * k, k * n
    batch = _prod(batch_shape)
    return self._gemm(a, b, False, False, m, n, k, k, n, batch, stride_a, stride_b,
                      out_shape=tuple(batch_shape) + (m, n), alias=alias)

  def _broadcast_to(self, t, shape):
    if tuple(t.shape) == tuple(shape):
      return t
    pad = len(shape) - t.ndim
    strides = [0] * pad + _row_major_strides(t.shape)
    for d, (have, want) in enumerate(zip((1,) * pad + tuple(t.shape), shape)):
      if have != want:
        if have != 1:
          raise ValueError(f"operands could not be broadcast together with shapes {t.shape} {shape}")
        strides[d] = 0
    return self._strided_copy(t, shape, strides, 0)

  def einsum(self, expression, *tensors, optimize=True):  # pylint: disable=unused-argument
    """einsum through the backend's own pairwise contraction (no NumPy compute)."""
    from tensornetwork_amd.ncon import einsum as _einsum  # pylint: disable=import-outside-toplevel
    return _einsum(expression, *[self._as_tensor(t) for t in tensors], backend=self)

  # --------------------------------------------------------------- reductions
  def trace(self, tensor, offset=0, axis1=-2, axis2=-1):
    tensor = self._as_tensor(tensor)
    self._check_num(tensor, "trace")
    nd = tensor.ndim
    if nd < 2:
      raise ValueError("diag requires an array of at least two dimensions")
    ax1, ax2 = axis1 % nd, axis2 % nd
    if ax1 == ax2:
      raise ValueError("axis1 and axis2 cannot be the same")
    rest = [i for i in range(nd) if i not in (ax1, ax2)]
    t = self.transpose(self._canonical(tensor), rest + [ax1, ax2])
    if t.code == _lib.I32:
      t = self.cast(t, _lib.I64)              # np.trace accumulates (and returns) int64 for narrower integers, like np.sum
    outer = _prod(t.shape[:-2])
    out = DeviceTensor.empty(t.shape[:-2], t.code, _sum_alias(t))
    _lib.check(self.lib.tnh_trace_last2(_vp(out), _vp(t), outer, t.shape[-2], t.shape[-1],
                                        int(offset), t.code), "tnh_trace_last2")
    return out

  def sum(self, tensor, axis=None, keepdims=False):
    tensor = self._as_tensor(tensor)
    self._check_num(tensor, "sum")
    nd = tensor.ndim
    if axis is None:
      axes = list(range(nd))
    else:
      if isinstance(axis, numbers.Integral):
        axis = (axis,)
      axes = sorted({int(x) % nd if nd else int(x) for x in tuple(axis)})
    kept = [i for i in range(nd) if i not in axes]
    final_shape = tuple(1 if i in axes else tensor.shape[i] for i in range(nd)) if keepdims else \
        tuple(tensor.shape[i] for i in kept)
    if not axes:
      return tensor.view(final_shape)
    tensor = self._canonical(tensor)
    if tensor.code == _lib.I32:
      tensor = self.cast(tensor, _lib.I64)    # np.sum accumulates (and returns) int64 for narrower integers
    contiguous_run = axes == list(range(axes[0], axes[-1] + 1))
    if contiguous_run:
      outer = _prod(tensor.shape[:axes[0]])
      red = _prod(tensor.shape[axes[0]:axes[-1] + 1])
      inner = _prod(tensor.shape[axes[-1] + 1:])
      src = tensor
    else:
      src = self.transpose(tensor, kept + axes)
      outer = _prod(tensor.shape[i] for i in kept)
      red = _prod(tensor.shape[i] for i in axes)
      inner = 1
    out = DeviceTensor.empty(final_shape, tensor.code, _sum_alias(tensor))
    _lib.check(self.lib.tnh_sum_mid(_vp(out), _vp(src), outer, red, inner, tensor.code), "tnh_sum_mid")
    return out

  def norm(self, tensor):
    tensor = self._as_tensor(tensor)
    self._check_num(tensor, "norm")
    if tensor.code in _INT_CODES:
      tensor = self.cast(tensor, _lib.F64)    # np.linalg.norm of an integer array is a float64
    out = DeviceTensor.empty((), tensor.code)
    _lib.check(self.lib.tnh_norm(_vp(out), _vp(tensor), tensor.size, tensor.code), "tnh_norm")
    if tensor.is_complex:
      return self._unary(_lib.OP_REAL, out)
    return out

  # --------------------------------------------------------------- elementwise
  def _unary(self, op, tensor):
    tensor = self._as_tensor(tensor)
    self._check_num(tensor, "elementwise math")
    if tensor.code in _INT_CODES and op in (_lib.OP_SQRT, _lib.OP_EXP, _lib.OP_LOG, _lib.OP_SIN, _lib.OP_COS):
      tensor = self.cast(tensor, _lib.F64)    # NumPy evaluates these on integers in float64
    if op in (_lib.OP_ABS, _lib.OP_SIGN):
      tensor = self._canonical(tensor)
    to_real = tensor.is_complex and op in (_lib.OP_ABS, _lib.OP_REAL, _lib.OP_IMAG)
    out = DeviceTensor.empty(tensor.shape, _REAL_OF[tensor.code] if to_real else tensor.code, tensor.alias)
    _lib.check(self.lib.tnh_unary(op, _vp(out), _vp(tensor), tensor.size, tensor.code), "tnh_unary")
    return out

  def sqrt(self, tensor):
    return self._unary(_lib.OP_SQRT, tensor)

  def conj(self, tensor):
    tensor = self._as_tensor(tensor)
    if not tensor.is_complex:
      if tensor.alias is not None and tensor.alias.kind == "b":
        return self.cast(tensor, np.int8)     # np.conj has no bool loop: NumPy answers in int8
      return tensor
    return self._unary(_lib.OP_CONJ, tensor)

  def abs(self, tensor):
    return self._unary(_lib.OP_ABS, tensor)

  def real(self, tensor):
    """Real part (a real tensor is returned as is)."""
    tensor = self._as_tensor(tensor)
    return self._unary(_lib.OP_REAL, tensor) if tensor.is_complex else tensor

  def imag(self, tensor):
    """Imaginary part (zeros for a real tensor)."""
    tensor = self._as_tensor(tensor)
    return self._unary(_lib.OP_IMAG, tensor) if tensor.is_complex else self.zeros(tensor.shape, tensor.dtype)

  def sign(self, tensor):
    return self._unary(_lib.OP_SIGN, tensor)

  def exp(self, tensor):
    return self._unary(_lib.OP_EXP, tensor)

  def log(self, tensor):
    return self._unary(_lib.OP_LOG, tensor)

  def sin(self, tensor):
    return self._unary(_lib.OP_SIN, tensor)

  def cos(self, tensor):
    return self._unary(_lib.OP_COS, tensor)

  @staticmethod
  def _is_scalar(x):
    return isinstance(x, numbers.Number) or (isinstance(x, np.ndarray) and x.ndim == 0) or \
        isinstance(x, np.generic)

  def _binary(self, op, x, y):
    xs, ys = self._is_scalar(x), self._is_scalar(y)
    if xs and ys:
      raise TypeError("at least one operand must be a tensor")
    if xs or ys:
      t = self._as_tensor(y if xs else x)
      sv = x if xs else y
      s = complex(sv)
      self._check_num(t, "arithmetic")
      if t.code == _lib.BF16:
        if s.imag != 0.0:
          t = self.cast(t, _lib.C64)          # no NumPy dtype to ask: bf16 stays bf16, a complex scalar makes complex64
      else:
        # NumPy's promotion (NEP 50): a Python scalar is weakly typed -- it keeps the tensor's dtype unless its KIND
        # is higher (bool < int < float < complex), then the default dtype of that kind at the tensor's precision
        # (bool (op) 3 -> int64, int32 (op) True -> int32, int (op) 2.5 -> float64, float32 (op) 1j -> complex64);
        # a NumPy scalar is strongly typed.  np.result_type implements both.
        res = np.result_type(np.dtype(t.dtype), sv)
        if op == _lib.OP_DIV and res.kind in "iub":
          res = np.dtype(np.float64)          # true division of integers is float64
        if res != np.dtype(t.dtype):
          t = self.cast(t, res)
      code = t.code
      out = DeviceTensor.empty(t.shape, code, t.alias)
      _lib.check(self.lib.tnh_binary_scalar(op, _vp(out), _vp(t), s.real, s.imag, 1 if xs else 0,
                                            t.size, code), "tnh_binary_scalar")
      return out
    a, b = self._as_tensor(x), self._as_tensor(y)
    ires = _int_result(a, b)
    code, alias = ires if ires is not None else (_promote(a.code, b.code), None)
    if op == _lib.OP_DIV and code in _INT_CODES:
      code, alias = _lib.F64, None            # NumPy: int / int is a float64 true division
    a, b = self.cast(a, code), self.cast(b, code)
    self._check_num(a, "arithmetic")
    try:
      shape = tuple(np.broadcast_shapes(a.shape, b.shape))
    except ValueError as exc:
      raise ValueError(f"operands could not be broadcast together with shapes "
                       f"{a.shape} {b.shape}") from exc

    def bstrides(t):
      pad = len(shape) - t.ndim
      st = [0] * pad + _row_major_strides(t.shape)
      dims = (1,) * pad + tuple(t.shape)
      return [0 if dims[d] == 1 and shape[d] != 1 else st[d] for d in range(len(shape))]

    out = DeviceTensor.empty(shape, code, alias)
    kshape, sa, sb = list(shape), bstrides(a), bstrides(b)
    if len(kshape) > MAX_KERNEL_RANK:
      # axes both operands (and the result) walk as one run are one axis to the kernel
      kshape, (sa, sb, _) = _coalesce_strided(kshape, sa, sb, _row_major_strides(shape))
      if len(kshape) > MAX_KERNEL_RANK:
        raise NotImplementedError(f"a broadcast with {len(kshape)} independent axes (one launch indexes "
                                  f"{MAX_KERNEL_RANK})")
    _lib.check(self.lib.tnh_binary(op, _vp(out), _vp(a), _vp(b), len(kshape), _lib.i64_array(kshape),
                                   _lib.i64_array(sa), _lib.i64_array(sb), code),
               "tnh_binary")
    return out

  def addition(self, tensor1, tensor2):
    return self._binary(_lib.OP_ADD, tensor1, tensor2)

  def subtraction(self, tensor1, tensor2):
    return self._binary(_lib.OP_SUB, tensor1, tensor2)

  def multiply(self, tensor1, tensor2):
    return self._binary(_lib.OP_MUL, tensor1, tensor2)

  def divide(self, tensor1, tensor2):
    return self._binary(_lib.OP_DIV, tensor1, tensor2)

  def power(self, a, b):
    return self._binary(_lib.OP_POW, a, b)

  def broadcast_right_multiplication(self, tensor1, tensor2):
    tensor2 = self._as_tensor(tensor2)
    if len(tensor2.shape) != 1:
      raise ValueError("only order-1 tensors are allowed for `tensor2`,"
                       " found `tensor2.shape = {}`".format(tensor2.shape))
    return self._binary(_lib.OP_MUL, tensor1, tensor2)

  def broadcast_left_multiplication(self, tensor1, tensor2):
    tensor1 = self._as_tensor(tensor1)
    tensor2 = self._as_tensor(tensor2)
    if len(tensor1.shape) != 1:
      raise ValueError("only order-1 tensors are allowed for `tensor1`,"
                       " found `tensor1.shape = {}`".format(tensor1.shape))
    t1_broadcast_shape = self.shape_concat(
        [self.shape_tensor(tensor1), [1] * (len(tensor2.shape) - 1)], axis=-1)
    return self._binary(_lib.OP_MUL, tensor2, self.reshape(tensor1, t1_broadcast_shape))

  # ------------------------------------------------------------ initialisation
  def _fill(self, shape, dtype, re, im=0.0):
    dtype = dtype if dtype is not None else np.float64
    code, alias = storage_of(dtype)
    self.lib  # pylint: disable=pointless-statement
    out = DeviceTensor.empty(shape, code, alias)
    _lib.check(self.lib.tnh_fill(_vp(out), float(re), float(im), out.size, code), "tnh_fill")
    return out

  def ones(self, shape, dtype=None):
    return self._fill(tuple(shape), dtype, 1.0)

  def zeros(self, shape, dtype=None):
    return self._fill(tuple(shape), dtype, 0.0)

  def eye(self, N, dtype=None, M=None):
    dtype = dtype if dtype is not None else np.float64
    code, alias = storage_of(dtype)
    self.lib  # pylint: disable=pointless-statement
    cols = int(N) if M is None else int(M)
    out = DeviceTensor.empty((int(N), cols), code, alias)
    _lib.check(self.lib.tnh_eye(_vp(out), int(N), cols, code), "tnh_eye")
    return out

  def randn(self, shape, dtype=None, seed=None):
    # Same host generator and call order as numpy_backend.py:137-149, so that a
    # seeded network is bit-identical to the NumPy backend's before upload.
    if seed:
      np.random.seed(seed)
    dtype = dtype if dtype is not None else np.float64
    if dtype is bfloat16:
      return self.to_bfloat16(np.random.randn(*shape).astype(np.float32))
    if np.dtype(dtype) in (np.dtype(np.complex128), np.dtype(np.complex64)):
      host = np.random.randn(*shape).astype(dtype) + 1j * np.random.randn(*shape).astype(dtype)
    else:
      host = np.random.randn(*shape).astype(dtype)
    return self.convert_to_tensor(np.asarray(host))

  def random_uniform(self, shape, boundaries=(0.0, 1.0), dtype=None, seed=None):
    if seed:
      np.random.seed(seed)
    dtype = dtype if dtype is not None else np.float64
    lo, hi = boundaries
    if dtype is bfloat16:
      return self.to_bfloat16(np.random.uniform(lo, hi, shape).astype(np.float32))
    if np.dtype(dtype) in (np.dtype(np.complex128), np.dtype(np.complex64)):
      host = np.random.uniform(lo, hi, shape).astype(dtype) + \
          1j * np.random.uniform(lo, hi, shape).astype(dtype)
    else:
      host = np.random.uniform(lo, hi, shape).astype(dtype)
    return self.convert_to_tensor(np.asarray(host))

  def device_random(self, shape, dtype=np.float32, seed=0, normal=True, a=0.0, b=1.0):
    """Synthetic operand generated directly in HBM (benchmarks / large tests).

    Not NumPy's stream -- use ``randn`` for reference-identical values."""
    code = tnh_dtype(dtype)
    self.lib  # pylint: disable=pointless-statement
    out = DeviceTensor.empty(tuple(shape), code)
    _lib.check(self.lib.tnh_random(_vp(out), out.size, code, int(seed), 1 if normal else 0, float(a),
                                   float(b)), "tnh_random")
    return out

  # ------------------------------------------------------------ diag helpers
  def diagflat(self, tensor, k=0):
    tensor = self._as_tensor(tensor)
    n = tensor.size
    side = n + abs(int(k))
    out = DeviceTensor.empty((side, side), tensor.code, tensor.alias)
    _lib.check(self.lib.tnh_memset(_vp(out), 0, out.nbytes), "tnh_memset")
    offset = int(k) if k >= 0 else -int(k) * side
    _lib.check(self.lib.tnh_strided_scatter(_vp(out), _vp(tensor), 1, _lib.i64_array((n,)),
                                            _lib.i64_array((side + 1,)), offset, tensor.itemsize),
               "tnh_strided_scatter")
    return out

  def diagonal(self, tensor, offset=0, axis1=-2, axis2=-1):
    tensor = self._as_tensor(tensor)
    nd = tensor.ndim
    if nd < 2:
      raise ValueError("diag requires an array of at least two dimensions")
    ax1, ax2 = axis1 % nd, axis2 % nd
    if ax1 == ax2:
      raise ValueError("axis1 and axis2 cannot be the same")
    st = _row_major_strides(tensor.shape)
    n, m = tensor.shape[ax1], tensor.shape[ax2]
    if offset >= 0:
      length, start = max(min(n, m - offset), 0), offset * st[ax2]
    else:
      length, start = max(min(n + offset, m), 0), -offset * st[ax1]
    rest = [i for i in range(nd) if i not in (ax1, ax2)]
    shape = [tensor.shape[i] for i in rest] + [length]
    strides = [st[i] for i in rest] + [st[ax1] + st[ax2]]
    return self._strided_copy(tensor, shape, strides, start if length else 0)

  # ------------------------------------------------------------ decompositions
  def svd(self, tensor, pivot_axis=-1, max_singular_values=None, max_truncation_error=None,
          relative=False):
    """Truncated SVD (abstract_backend.py:79-137; rule of decompositions.py:21-74).

    Two device paths, same truncation rule (decompositions.py:38-57, restated on the host on the singular values):

      * band path (K7b, `_svd_band`; f32 / bf16 / f16 / f64 with min(m, n) >= `svd_band_min`, complex64 / complex128
        through the real embedding): band reduction, spectrum slicing for the values, inverse iteration for the KEPT
        vectors only, back-transformation.  Every call shape (max_singular_values, max_truncation_error, both, neither).
      * one-sided block Jacobi (K7; every other shape, and the fall-back): all singular values, then only the kept
        vectors are emitted.  complex inputs use unitary plane rotations, in 64-row blocks on the matrix cores for
        min(m, n) > 64 like the real ones; exactly rank-deficient complex inputs get a completed basis.

    Which one ran is in `last_svd_path` after the call.  The band path reports numerically rank-deficient panels /
    unconverged vectors through a status word; the call then falls back to Jacobi, and a shape that reports twice in
    a row skips the band path for min(2^f, 64) calls (`svd_band_policy()` shows the state, `reset_svd_band_policy()`
    clears it, `svd_band_backoff = False` switches the skipping off; the state lives in this backend object).  Both
    paths obey the same rule; they differ in the accuracy of the DISCARDED values `s_rest` (band: 20-bit brackets,
    5e-7 s_1; Jacobi: full precision).
    """
    tensor = self._as_tensor(tensor)
    self._check_float(tensor, "svd")
    left_dims = tensor.shape[:pivot_axis]
    right_dims = tensor.shape[pivot_axis:]
    m, n = _prod(left_dims), _prod(right_dims)
    orig_code = tensor.code
    work_code = tensor.code if tensor.code in (_lib.F32, _lib.F64, _lib.C64, _lib.C128) else _lib.F32
    real_code = _REAL_OF.get(work_code, work_code)     # singular values come out real
    mat = self.cast(tensor, work_code).view((m, n))
    r = min(m, n)
    self.last_svd_path = "jacobi"

    if work_code in (_lib.F32, _lib.F64) and getattr(self, "svd_band", True) and \
        (work_code == _lib.F32 or getattr(self, "svd_band_f64", True)):
      done = self._svd_band(mat, m, n, max_singular_values, max_truncation_error, relative)
      if done is not None:
        u, s, vh, s_rest = done
        keep = s.shape[0]
        if orig_code != work_code:
          u, vh = self.cast(u, orig_code), self.cast(vh, orig_code)
        if orig_code != real_code:
          s, s_rest = self.cast(s, orig_code), self.cast(s_rest, orig_code)
        return u.view(tuple(left_dims) + (keep,)), s, vh.view((keep,) + tuple(right_dims)), s_rest

    if work_code in (_lib.C64, _lib.C128) and getattr(self, "svd_band", True) and \
        (work_code == _lib.C64 or getattr(self, "svd_band_f64", True)):
      done = self._svd_complex_band(mat, m, n, max_singular_values, max_truncation_error, relative)
      if done is not None:
        u, s, vh, s_rest = done
        keep = s.shape[0]
        s, s_rest = self.cast(s, orig_code), self.cast(s_rest, orig_code)      # decompositions.py:58-62
        return u.view(tuple(left_dims) + (keep,)), s, vh.view((keep,) + tuple(right_dims)), s_rest

    nbytes = ctypes.c_size_t(0)
    _lib.check(self.lib.tnh_svd_work_bytes(work_code, m, n, ctypes.byref(nbytes)), "tnh_svd_work_bytes")
    work = DeviceTensor.empty((max(nbytes.value, 8) // 8 + 1,), _lib.F64)
    s_all = DeviceTensor.empty((r,), real_code)
    sweeps = ctypes.c_int(0)
    # top-k mode: a call that keeps at most half of the spectrum does not need the accumulated
    # rotations of the other side -- its k vectors come from A by one GEMM (tnh_svd_vectors_topk)
    topk = (max_singular_values is not None and 2 * int(max_singular_values) <= r and
            getattr(self, "svd_topk", True))
    mode = ctypes.c_int(0)
    if topk:
      _lib.check(self.lib.tnh_svd_factor_topk(work_code, m, n, _vp(mat), _vp(s_all), _vp(work),
                                              ctypes.byref(sweeps), ctypes.byref(mode)), "tnh_svd_factor_topk")
    else:
      _lib.check(self.lib.tnh_svd_factor(work_code, m, n, _vp(mat), _vp(s_all), _vp(work),
                                         ctypes.byref(sweeps)), "tnh_svd_factor")
    self.last_svd_sweeps = sweeps.value

    if max_singular_values is None:
      max_singular_values = r
    s_host = None
    if max_truncation_error is not None or mode.value == 1:
      s_host = s_all.numpy().astype(np.float64)
    if max_truncation_error is not None:
      # cumulative norms of the singular values in ascending order
      trunc_errs = np.sqrt(np.cumsum(np.square(s_host[::-1])))
      abs_err = max_truncation_error * (s_host[0] if r else 0.0) if relative else max_truncation_error
      num_sing_vals_err = int(np.count_nonzero(trunc_errs > abs_err))
    else:
      num_sing_vals_err = max_singular_values
    keep = int(min(max_singular_values, num_sing_vals_err, r))
    keep = max(keep, 0)

    u = DeviceTensor.empty((m, keep), work_code)
    vh = DeviceTensor.empty((keep, n), work_code)
    if mode.value == 1 and keep > 0 and not s_host[keep - 1] > 0.0:
      # exactly rank-deficient inside the kept block: the orthogonalised side itself has zero rows, which
      # only the accumulating path completes to an orthonormal basis (rare: zero / low-rank inputs)
      _lib.check(self.lib.tnh_svd_factor(work_code, m, n, _vp(mat), _vp(s_all), _vp(work),
                                         ctypes.byref(sweeps)), "tnh_svd_factor")
      mode.value = 0
    if mode.value == 1:
      _lib.check(self.lib.tnh_svd_vectors_topk(work_code, m, n, _vp(mat), _vp(work), _vp(s_all), keep, _vp(u),
                                               _vp(vh)), "tnh_svd_vectors_topk")
      if keep > 0 and not s_host[keep - 1] * 100.0 >= s_host[0]:
        # Not all kept triplets are leading ones: (A v_k) / s_k carries eps * s_1 / s_k of noise, i.e. the
        # recovered vectors lose orthogonality.  Re-orthonormalise them with the Householder QR (K9) of
        # Y = A Vh_k^T (resp. A^T U_k), WITHOUT the division: column k of Y is s_k u_k + O(eps s_1), QR
        # orthogonalises it against the more accurate earlier columns, and a numerically zero column
        # gets an orthonormal completion -- what LAPACK returns there too.  U S Vh stays within
        # O(eps s_1) of A_k, the backward error of any SVD.
        def unit(q_, r_):
          sgn = self.sign(self.diagonal(r_))
          sgn = self._binary(_lib.OP_ADD, sgn, self._binary(_lib.OP_SUB, 1.0, self.abs(sgn)))
          return self._binary(_lib.OP_MUL, q_, sgn)
        if m <= n:
          u = unit(*self._qr_matrix(self._tensordot_impl(mat, vh, [[1], [1]], None, None)[0]))
        else:
          vh = self.transpose(unit(*self._qr_matrix(self._tensordot_impl(mat, u, [[0], [0]], None, None)[0])), (1, 0))
    else:
      _lib.check(self.lib.tnh_svd_vectors(work_code, m, n, _vp(work), keep, _vp(u), _vp(vh)),
                 "tnh_svd_vectors")
    s = self.getitem(s_all, slice(0, keep))
    s_rest = self.getitem(s_all, slice(keep, r))
    if orig_code != work_code:
      u, vh = self.cast(u, orig_code), self.cast(vh, orig_code)
    if orig_code != real_code:    # decompositions.py:58-62: s is recast to the tensor's dtype (complex included)
      s, s_rest = self.cast(s, orig_code), self.cast(s_rest, orig_code)
    u = u.view(tuple(left_dims) + (keep,))
    vh = vh.view((keep,) + tuple(right_dims))
    return u, s, vh, s_rest

  # smallest min(m, n) the band path takes: measured 512^2 keep 32: band 3.9 ms (Gaussian and graded), block Jacobi
  # 9.5 / 17.8 ms; 768^2: 5.9 vs 14.6 ms (profiles/r03_svd_small_n.txt)
  svd_band_min = 512
  last_svd_path = None
  last_svd_band_status = 0
  _svd_band_failed = set()      # tall shapes whose last band call reported a status: read it early next time
  _svd_band_backoff = {}        # (dtype, mm, nn) -> (consecutive reports, calls still to skip)

  svd_band_backoff = True       # skip the band path for shapes that keep reporting (see svd's docstring)
  # Rates of the lowering's cost rule (calibrated on one box family in round 5 -- boxes differ by
  # 13 % in clock under the same power cap -- so they are attributes a deployment can re-calibrate, not literals):
  model_gemm_flops = 1.45e15       # flop/s of the bf16 ping-pong GEMM on random data under the 1400 W cap
  model_k1_bytes_per_s = 5.0e12    # read + write rate of a K1 pass
  model_launch_s = 6.0e-6          # one more dependent launch
  k_blocked_permutes = True      # tensordot: K1 passes of view-GEMM operands with rows of 1 MiB and more write the K-blocked form
  k_blocked_min_row_bytes = 1 << 20
  plan_cache = True              # tensordot: replay the lowering of a (shapes, axes, dtype, hints) seen before (False: plan every call)
  kmajor_tile_walk = True        # tensordot: the size-dependent cost rule for a k-major `b` the whole-K-tile lean loop reads
  kmajor_tile_walk_max_pitch = 1 << 16       # (elements between consecutive k rows of such a `b`)
  kmajor_tile_walk_penalty_per_gb = 0.03     # (fraction of the product per GB of the operand beyond 0.6 GB)
  complex_lowering = "embedded"   # planned complex tensordot (>= 2^18 flops): "embedded" = tnh_complex_expand + ONE real
                                  # GEMM of M x 2N x 2K (`_complex_gemm`); "native" = ONE complex tnh_gemm on the operands
                                  # where they lie (the mfma_c64_* / mfma_c128_* kernels; measured in profiles/complex_native.md)
  kmajor_inplace_penalty = 0.10  # tensordot: what reading a k-major operand in place costs the product (0: always in place
                                 # below inplace_max_bytes, the rule of rounds 2-4)
  inplace_strided_max_bytes = 4 << 30
  inplace_strided_big = True    # tensordot: read K-contiguous two-level views above inplace_max_bytes in place when their
                                # contraction runs are multiples of 64 (False: the round 2-4 gate copies them when the
                                # product is compute-heavy)

  def svd_band_policy(self):
    """The band path's back-off state: {(dtype code, rows, cols): {"consecutive_reports", "calls_still_skipped"}} and
    the shapes whose status word is read early.  Empty = every eligible call tries the band path."""
    return {"backoff": {k: {"consecutive_reports": f, "calls_still_skipped": sk} for k, (f, sk) in self._svd_band_backoff.items()},
            "status_read_early_for": sorted(self._svd_band_failed), "enabled": bool(self.svd_band_backoff)}

  def reset_svd_band_policy(self):
    self._svd_band_failed.clear()
    self._svd_band_backoff.clear()

  # largest inverse-iteration workspace (the stored LDL^T factors: k * min(m, n) * 128 bytes) the band path asks for
  svd_band_max_factor_bytes = 24 << 30

  def _svd_band(self, mat, m, n, max_singular_values, max_truncation_error, relative):
    """K7b (tnh_svd_band_*): band reduction + spectrum slicing + inverse iteration, f32 and (round 4) f64,
    min(m, n) >= 512.

    Round 4: every call shape the reference makes (network_operations.py:130-255, 446-588) --
    `max_singular_values` alone, `max_truncation_error` alone (values first, k picked on the host by
    decompositions.py:38-57, then the vectors), neither (split_node_full_svd: k = min(m, n)) -- and any
    min(m, n): a side that is not a multiple of the 16-wide panels is padded (`_svd_band_pad`).  Returns
    (u (m, k), s (k,), vh (k, n), s_rest) or None when the device reports that the result must not be used
    (rank-deficient panel, clustered kept values, a kept value below 1e-6 s_1): the caller then runs the Jacobi
    path -- same truncation rule there."""
    r = min(m, n)
    self.last_svd_path = "jacobi"
    if r < self.svd_band_min:
      return None
    kmax = r if max_singular_values is None else min(int(max_singular_values), r)
    if kmax <= 0:
      return None
    wide = m < n
    mm, nn = (n, m) if wide else (m, n)
    a = self.transpose(mat, (1, 0)) if wide else mat
    pad, delta, mix = -r % 16, None, None
    if pad:
      a, delta, *mix = self._svd_band_pad(a, mm, nn, pad)
      if a is None:
        return None
    pick = None
    if max_truncation_error is not None:
      def pick(s_host):      # decompositions.py:38-57 on A's values (the `pad` leaders of a padded spectrum are not A's)
        s_a = s_host[pad:]
        trunc_errs = np.sqrt(np.cumsum(np.square(s_a[::-1])))
        abs_err = max_truncation_error * (s_a[0] if s_a.size else 0.0) if relative else max_truncation_error
        return pad + int(min(kmax, int(np.count_nonzero(trunc_errs > abs_err)), r))
    done = self._svd_band_core(a, mm + pad, nn + pad, kmax + pad, pick)
    if done is None:
      return None
    uu, s, vvh, s_rest = done
    keep = s.shape[0] - pad
    if keep <= 0:
      return None
    if pad:
      # the `pad` leading triplets are (delta, e_i, e_i); anything else means the s_1 estimate was off by more than 2
      lead = np.asarray(self.getitem(s, slice(0, pad + 1)), dtype=np.float64)       # one read-back: the check below
      if np.any(np.abs(lead[:pad] - delta) > 1e-5 * delta) or not lead[pad] < delta * (1.0 - 1e-3):
        return None
      uu = self.getitem(uu, (slice(None), slice(pad, pad + keep)))
      vvh = self.getitem(vvh, slice(pad, pad + keep))
      uu, vvh = self._svd_band_unpad(uu, vvh, *mix)
      uu = self.getitem(uu, slice(0, mm))
      vvh = self.getitem(vvh, (slice(None), slice(0, nn)))
      s = self.getitem(s, slice(pad, pad + keep))
    if wide:      # A^T = U' S V'h  ->  A = V'h^T S U'^T
      u, vh = self.transpose(vvh, (1, 0)), self.transpose(uu, (1, 0))
    else:
      u, vh = uu, vvh
    self.last_svd_path = "band"
    self.last_svd_sweeps = 0
    return u, s, vh, s_rest

  def _svd_band_core(self, a, mm, nn, kmax, pick):
    """The device calls of the band path on a tall (mm >= nn) f32 / f64 matrix with nn % 16 == 0: factor (ALL values) ->
    number of kept triplets (`kmax`, or `pick(values on the host)`) -> vectors.  Returns (u (mm, keep), s (keep,),
    vh (keep, nn), s_rest (nn - keep,)) or None."""
    if pick is not None and nn * nn * self._svd_band_bytes_per_vector_row(a.code) > self.svd_band_max_factor_bytes:
      # k is only known after the values, and a work buffer for k = nn would be too large: values with the smallest
      # layout first, then the whole call again with the k they give (twice the factor stage; nn > 14000 only)
      first = self._svd_band_core(a, mm, nn, 4, None)
      if first is None:
        return None
      s_host = np.concatenate([np.asarray(first[1], dtype=np.float64), np.asarray(first[3], dtype=np.float64)])
      return self._svd_band_core(a, mm, nn, max(pick(s_host), 0), None)
    kmax = min(int(kmax), nn)
    # Back-off for shapes on which the path keeps reporting (round 4, measured on two-site DMRG: the splits in the
    # middle of the chain keep values below 1e-6 s_1, every one of them paid the band stages AND the Jacobi path:
    # 1.0 -> 1.8 s per sweep).  From the second consecutive report on (f = 2, 3, ...) a shape skips the band path
    # min(2^f, 64) times, then tries again; one success clears it.
    key = (a.code, mm, nn)
    fails, skip = self._svd_band_backoff.get(key, (0, 0))
    if skip > 0 and self.svd_band_backoff:
      self._svd_band_backoff[key] = (fails, skip - 1)
      self.last_svd_path = f"jacobi (band path skipped: {fails} consecutive status reports on this shape, {skip - 1} skips left)"
      return None
    kcap = nn if pick is not None else (kmax + 3) // 4 * 4
    if kmax <= 0 or kcap * nn * self._svd_band_bytes_per_vector_row(a.code) > self.svd_band_max_factor_bytes:
      return None
    if not self.lib.tnh_svd_band_supported(a.code, mm, nn, kcap):
      return None
    nbytes = ctypes.c_size_t(0)
    _lib.check(self.lib.tnh_svd_band_work_bytes(a.code, mm, nn, kcap, ctypes.byref(nbytes)), "tnh_svd_band_work_bytes")
    work = DeviceTensor.empty((nbytes.value // 8 + 1,), _lib.F64)
    s_all = DeviceTensor.empty((nn,), a.code)
    status = ctypes.c_int(0)
    # the status word of the factor stage is read back when the values are needed on the host anyway, and for a shape
    # whose last call failed (a rank-deficient input otherwise pays factor + vectors + Jacobi each time)
    check_now = pick is not None or (a.code, mm, nn) in self._svd_band_failed
    _lib.check(self.lib.tnh_svd_band_factor(a.code, mm, nn, _vp(a), _vp(s_all), _vp(work), kcap,
                                            ctypes.byref(status) if check_now else None), "tnh_svd_band_factor")
    if check_now and status.value:
      self.last_svd_band_status = status.value
      self._svd_band_backoff[key] = (fails + 1, 0 if fails == 0 else min(2 ** (fails + 1), 64))
      self.last_svd_path = f"jacobi (band path reported status {status.value} in its factor stage)"
      return None
    keep = kmax if pick is None else int(min(pick(s_all.numpy().astype(np.float64)), nn))
    if keep <= 0:
      return None
    kk = (keep + 3) // 4 * 4          # the back-transformation moves float4 columns; extra vectors are dropped
    uu = DeviceTensor.empty((mm, kk), a.code)
    vvh = DeviceTensor.empty((kk, nn), a.code)
    s_kept = DeviceTensor.empty((kk,), a.code)
    _lib.check(self.lib.tnh_svd_band_vectors(a.code, mm, nn, _vp(work), kcap, kk, _vp(uu), _vp(vvh), _vp(s_kept),
                                             ctypes.byref(status)), "tnh_svd_band_vectors")
    self.last_svd_band_status = status.value
    if status.value:
      self._svd_band_failed.add((a.code, mm, nn))
      self._svd_band_backoff[key] = (fails + 1, 0 if fails == 0 else min(2 ** (fails + 1), 64))
      self.last_svd_path = f"jacobi (band path reported status {status.value} in its vectors stage)"
      return None
    self._svd_band_failed.discard((a.code, mm, nn))
    self._svd_band_backoff.pop(key, None)
    if kk != keep:
      uu = self.getitem(uu, (slice(None), slice(0, keep)))
      vvh = self.getitem(vvh, slice(0, keep))
      s_kept = self.getitem(s_kept, slice(0, keep))
    # kept values: from the brackets the vectors stage refined to 2^-32 s_1; the discarded ones
    # keep the 20 bits every bracket gets (5e-7 s_1)
    return uu, s_kept, vvh, self.getitem(s_all, slice(keep, nn))

  @staticmethod
  def _svd_band_bytes_per_vector_row(code):
    """inverse-iteration workspace per kept vector and matrix row: the stored LDL^T factor (16 + 1 doubles) and the
    vector; the f64 path adds two more vector buffers (Newton-Schulz)"""
    return 128 + 16 + (16 if code == _lib.F64 else 0)

  def _svd_band_pad(self, a, mm, nn, pad):
    """nn not a multiple of the 16-wide panels: the band path runs on
        A'' = H_z blockdiag(A, delta I_pad) H_w,    H_x = I - 2 x x^T  (x a dense random unit vector),
    pad < 16, delta = 2 x a power-iteration estimate of s_1 (an estimate from below, so delta > s_1 unless it is off
    by more than a factor two -- the caller checks that on the returned values).  A'' has the singular values of A
    plus `pad` values delta that lead the spectrum, and singular vectors H_z [u; 0], H_w [v; 0]: the call asks for
    `pad` more vectors, drops the first `pad` and undoes the two reflections (`_svd_band_unpad`).
    Why not zero padding: a zero column makes the last panel's Gram matrix singular, which the Cholesky-QR reports
    instead of processing.  Why the reflections: in the bare blockdiag form the reflectors of the delta columns are
    exact row swaps that leave whole ZERO rows in the next row panel (measured on the MI355X in round 4: status 25;
    reproduced in tools/svd_band_model.py) -- one dense reflection per side removes every exact zero, and the panels'
    Gram pivots stay where an unpadded matrix has them (model: 1e-3 ... 7e-7 of the largest, threshold 1e-9).
    Costs three extra passes over A, sixteen + two matrix-vector products, and a factor <= 2 in the absolute accuracy
    of the values (the brackets are relative to the largest value, now delta).
    Returns (A'', delta, z, w) or (None, None, None, None)."""
    npdt = np.float64 if a.code == _lib.F64 else np.float32
    x = self.cast(self.device_random((nn,), np.float32, seed=12345), a.code)
    for _ in range(8):
      y = self._tensordot_impl(a, x, [[1], [0]], None, None)[0]
      x = self._tensordot_impl(a, y, [[0], [0]], None, None)[0]
      x = self._binary(_lib.OP_DIV, x, self.norm(x))
    est = float(np.asarray(self.norm(self._tensordot_impl(a, x, [[1], [0]], None, None)[0])))
    if not np.isfinite(est) or est <= 0.0:
      return None, None, None, None
    delta = float(npdt(2.0 * est))
    big = DeviceTensor.empty((mm + pad, nn + pad), a.code)
    _lib.check(self.lib.tnh_memset(_vp(big), 0, big.nbytes), "tnh_memset")
    _lib.check(self.lib.tnh_strided_scatter(_vp(big), _vp(a), 2, _lib.i64_array((mm, nn)),
                                            _lib.i64_array((nn + pad, 1)), 0, a.itemsize), "tnh_strided_scatter")
    dvec = self._fill((pad,), npdt, delta)
    _lib.check(self.lib.tnh_strided_scatter(_vp(big), _vp(dvec), 1, _lib.i64_array((pad,)),
                                            _lib.i64_array((nn + pad + 1,)), mm * (nn + pad) + nn, a.itemsize),
               "tnh_strided_scatter")
    z = self.cast(self.device_random((mm + pad,), np.float32, seed=23456), a.code)
    z = self._binary(_lib.OP_DIV, z, self.norm(z))
    w = self.cast(self.device_random((nn + pad,), np.float32, seed=34567), a.code)
    w = self._binary(_lib.OP_DIV, w, self.norm(w))
    q = self._tensordot_impl(z, big, [[0], [0]], None, None)[0]                    # z^T A'
    big = self._binary(_lib.OP_SUB, big, self.outer_product(self._binary(_lib.OP_MUL, z, 2.0), q))
    p = self._tensordot_impl(big, w, [[1], [0]], None, None)[0]                    # (H_z A') w
    big = self._binary(_lib.OP_SUB, big, self.outer_product(self._binary(_lib.OP_MUL, p, 2.0), w))
    return big, delta, z, w

  def _svd_band_unpad(self, uu, vvh, z, w):
    """U' = H_z U'', V'^T = V''^T H_w for the vectors of the padded, reflected matrix (`_svd_band_pad`)."""
    c = self._tensordot_impl(z, uu, [[0], [0]], None, None)[0]                     # (k,)
    uu = self._binary(_lib.OP_SUB, uu, self.outer_product(self._binary(_lib.OP_MUL, z, 2.0), c))
    d = self._tensordot_impl(vvh, w, [[1], [0]], None, None)[0]                    # (k,)
    vvh = self._binary(_lib.OP_SUB, vvh, self.outer_product(self._binary(_lib.OP_MUL, d, 2.0), w))
    return uu, vvh

  def _svd_complex_band(self, mat, m, n, max_singular_values, max_truncation_error, relative):
    """complex64 / complex128 SVD of a large matrix through the REAL band path (f32 / f64).

    E = phi(conj(A)) (2m x 2n, real; phi(z) = [[re, im], [-im, re]], tnh_complex_expand) acts on interleaved
    (re, im) column vectors like A does on complex ones, so A = U S V^H  <=>  E = phi-form(U) (S x I_2) phi-form(V)^T:
    every singular value of A appears twice in E, and a real singular pair (x, y) of E is the complex pair
    (x[0::2] + i x[1::2],  y[0::2] + i y[1::2]) of A.  The band path returns an orthonormal basis of each doubled
    (or larger) value's subspace (cluster Gram-Schmidt); 2k real vectors hold k complex directions plus their
    multiples by i, from which k independent complex ones are picked and orthonormalised with the small (2k x 2k)
    complex Gram matrix on the host -- the same combination is applied to the right vectors, so A V = U S holds
    without a division.  Returns None outside the band path's range (the unitary-rotation Jacobi kernel then runs)."""
    r = min(m, n)
    self.last_svd_path = "jacobi"
    if 2 * r < self.svd_band_min:
      return None
    kmax = r if max_singular_values is None else min(int(max_singular_values), r)
    if kmax <= 0:
      return None
    ccode = mat.code                                         # complex64 -> f32 band path, complex128 -> f64
    rcode = _REAL_OF[ccode]
    rnp, cnp = (np.float32, np.complex64) if ccode == _lib.C64 else (np.float64, np.complex128)
    emb = DeviceTensor.empty((2 * m, 2 * n), rcode)
    _lib.check(self.lib.tnh_complex_expand(_vp(emb), _vp(mat), m, n, n, 1, 1, ccode), "tnh_complex_expand")
    done = self._svd_band(emb, 2 * m, 2 * n, 2 * kmax, None, False)
    self.last_svd_path = "jacobi"                            # until this method has an answer of its own
    if done is None:
      return None
    ur, sr, vrh, sr_rest = done                              # (2m, 2k), (2k,), (2k, 2n), (2r - 2k,)

    def pair_mean(x):                                        # every complex value appears twice: mean of each pair
      if x.shape[0] == 0:
        return x
      return self._binary(_lib.OP_MUL, self._binary(_lib.OP_ADD, self.getitem(x, slice(0, None, 2)),
                                                    self.getitem(x, slice(1, None, 2))), 0.5)

    keep = kmax
    s_kept_dev, s_rest_dev = pair_mean(sr), pair_mean(sr_rest)        # (kmax,), (r - kmax,): on the device
    if max_truncation_error is not None:
      # the truncation rule needs the values on the host (decompositions.py:38-57), as on every path
      s_c = np.concatenate([np.asarray(s_kept_dev, dtype=np.float64), np.asarray(s_rest_dev, dtype=np.float64)])
      trunc_errs = np.sqrt(np.cumsum(np.square(s_c[::-1])))
      abs_err = max_truncation_error * (s_c[0] if r else 0.0) if relative else max_truncation_error
      keep = int(min(kmax, int(np.count_nonzero(trunc_errs > abs_err)), r))
      if keep != kmax:
        s_all_dev = self.convert_to_tensor(s_c.astype(rnp))
        s_kept_dev, s_rest_dev = self.getitem(s_all_dev, slice(0, keep)), self.getitem(s_all_dev, slice(keep, r))
    if keep <= 0:
      return None
    k2 = 2 * keep

    def as_complex(x, rows, cols, ld):
      # complex[i, j] = x[2 i, j] + i x[2 i + 1, j]: one strided gather into interleaved (re, im)
      out = DeviceTensor.empty((rows, cols), ccode)
      _lib.check(self.lib.tnh_strided_copy(_vp(out), _vp(x), 3, _lib.i64_array((rows, cols, 2)),
                                           _lib.i64_array((2 * ld, 1, ld)), 0, 4 if rcode == _lib.F32 else 8),
                 "tnh_strided_copy")
      return out

    zu = as_complex(ur, m, k2, 2 * kmax)                     # candidates for U: m x 2k (first 2 keep columns)
    vr = self.transpose(vrh, (1, 0))                         # (2n, 2k)
    zv = as_complex(vr, n, k2, 2 * kmax)
    # k independent complex directions among the 2k candidates.  The two real vectors of a pair span ONE complex
    # line and different pairs are orthogonal, so the even-numbered candidates Z_e are orthonormal up to the real
    # path's own error; one Newton-Schulz step  Z_e (1.5 I - 0.5 Z_e^H Z_e)  on the DEVICE polishes them (round 4: no
    # host LAPACK in this path any more), and the same coefficients go onto the right vectors, so that A V = U S holds
    # without a division.  The one read-back is the check at the end: |Z_e^H Z_e - I| -- large only when a complex
    # value is itself degenerate (real clusters of four and more, where the even candidates can be dependent).
    even = (slice(None), slice(0, k2, 2))
    zue, zve = self.getitem(zu, even), self.getitem(zv, even)
    eye = self.eye(keep, dtype=cnp)
    gram = self._tensordot_impl(self.conj(zue), zue, [[0], [0]], None, None)[0]           # keep x keep
    dev = float(np.asarray(self.norm(self._binary(_lib.OP_SUB, gram, eye))).real)
    if np.isfinite(dev) and dev < 0.1 and not self.svd_complex_force_cluster_path:
      coef_dev = self._binary(_lib.OP_SUB, self._binary(_lib.OP_MUL, eye, 1.5), self._binary(_lib.OP_MUL, gram, 0.5))
      u = self._tensordot_impl(zue, coef_dev, [[1], [0]], None, None)[0]                  # m x keep
      v = self._tensordot_impl(zve, coef_dev, [[1], [0]], None, None)[0]                  # n x keep
    else:
      # degenerate complex values (or `svd_complex_force_cluster_path`, which the GPU tests set to cover this branch):
      # greedy Gram-Schmidt over all 2k candidates on the (2k x 2k) Gram matrix -- host arithmetic on a small matrix
      g = np.asarray(self._tensordot_impl(self.conj(zu), zu, [[0], [0]], None, None)[0]).astype(np.complex128)
      basis = self._independent_directions(g, keep)
      if basis is None:
        return None
      cdev = self.convert_to_tensor(basis.astype(cnp))
      u = self._tensordot_impl(zu, cdev, [[1], [0]], None, None)[0]               # m x keep
      v = self._tensordot_impl(zv, cdev, [[1], [0]], None, None)[0]               # n x keep
    vh = self.conj(self.transpose(v, (1, 0)))
    s_dev, s_rest = s_kept_dev, s_rest_dev
    self.last_svd_path = "band (complex via the real embedding)"
    return u, s_dev, vh, s_rest

  svd_complex_force_cluster_path = False     # tests: take the degenerate-value branch of _svd_complex_band always

  @staticmethod
  def _independent_directions(gram, keep):
    """`keep` coefficient vectors c (columns of the result) such that the combinations Z c of the candidates Z with
    Gram matrix `gram` = Z^H Z are orthonormal: greedy Gram-Schmidt in the Gram metric over the candidates in their
    order, a candidate whose remainder has squared norm <= 1/4 is dependent on the earlier ones and skipped.  None
    when fewer than `keep` independent directions exist."""
    g = np.asarray(gram, dtype=np.complex128)
    n = g.shape[0]
    basis = []
    for j in range(n):
      c = np.zeros(n, dtype=np.complex128)
      c[j] = 1.0
      for bvec in basis:
        c = c - bvec * (bvec.conj() @ g @ c)
      nrm2 = float(np.real(c.conj() @ g @ c))
      if nrm2 > 0.25:
        basis.append(c / np.sqrt(nrm2))
        if len(basis) == keep:
          return np.stack(basis, axis=1)
    return None

  complex_qr = "embedded"   # complex qr / rq: "embedded" = the real tnh_qr on the 2m x 2n embedding (`_qr_complex`);
                            # "native" = ONE tnh_qr call on the interleaved complex matrix (tnh_qr_complex.hip; no
                            # read-back, capturable; measured in profiles/qr_complex.md)
  last_qr_path = None       # "real" / "embedded complex" / "native complex" after a qr / rq (or an svd's internal QR)

  def _qr_matrix(self, mat):
    """Thin Householder QR of a device matrix -> (q (m, k), r (k, n)); complex matrices follow `complex_qr`."""
    if mat.is_complex:
      if self.complex_qr not in ("embedded", "native"):
        raise ValueError(f"complex_qr must be 'embedded' or 'native', got {self.complex_qr!r}")
      if self.complex_qr == "embedded":
        q, r = self._qr_complex(mat)
        self.last_qr_path = "embedded complex"
        return q, r
      q, r = self._qr_device(mat)
      # zgeqrf leaves R's diagonal real with LAPACK's sign: the same gauge step as the embedded path (diag(R) >= 0, a
      # zero diagonal keeps +1; the factor is real, so it is its own conjugate on R's rows)
      sgn = self.sign(self.real(self.diagonal(r)))
      sgn = self._binary(_lib.OP_ADD, sgn, self._binary(_lib.OP_SUB, 1.0, self.abs(sgn)))
      q = self._binary(_lib.OP_MUL, q, sgn)
      r = self._binary(_lib.OP_MUL, self.reshape(sgn, (sgn.shape[0], 1)), r)
      self.last_qr_path = "native complex"
      return q, r
    q, r = self._qr_device(mat)
    self.last_qr_path = "real"
    return q, r

  def _qr_device(self, mat):
    """One tnh_qr call on a device matrix of a dtype the kernel takes (f32 / f64 / complex64 / complex128)."""
    m, n = mat.shape
    k = min(m, n)
    nbytes = ctypes.c_size_t(0)
    _lib.check(self.lib.tnh_qr_work_bytes(mat.code, m, n, ctypes.byref(nbytes)), "tnh_qr_work_bytes")
    work = DeviceTensor.empty((max(nbytes.value, 8) // 8 + 1,), _lib.F64)
    q = DeviceTensor.empty((m, k), mat.code)
    r = DeviceTensor.empty((k, n), mat.code)
    _lib.check(self.lib.tnh_qr(mat.code, m, n, _vp(mat), _vp(q), _vp(r), _vp(work)), "tnh_qr")
    return q, r

  def _qr_complex(self, mat):
    """Thin QR of a complex matrix through the REAL Householder kernels.

    phi(z) = [[re, -im], [im, re]] is a ring homomorphism, so the interleaved real embedding
    phi(A) (2m x 2n) satisfies phi(A) = phi(Q) phi(R); phi(R) is upper triangular with the real
    non-negative diagonal of R doubled, and a full-column-rank matrix has exactly one QR with a
    positive diagonal -- hence the real QR of phi(A), phase-fixed to a non-negative diagonal, IS
    (phi(Q), phi(R)).  Column 2j of phi(X) is (re, im) of column j of X, which is read back with one
    strided gather.  R therefore always comes out with a real non-negative diagonal (a valid QR;
    LAPACK's complex reflectors fix a different phase).  Exactly rank-deficient inputs lose the
    uniqueness argument; the all-zero matrix still gives Q = 1, R = 0 like LAPACK."""
    m, n = mat.shape
    k = min(m, n)
    real = _REAL_OF[mat.code]
    emb = DeviceTensor.empty((2 * m, 2 * n), real)
    _lib.check(self.lib.tnh_complex_expand(_vp(emb), _vp(mat), m, n, n, 1, 1, mat.code), "tnh_complex_expand")
    qh, rh = self._qr_matrix(emb)                            # (2m x 2k), (2k x 2n)
    # flip reflector signs so that diag(R) >= 0; a zero diagonal entry (tau = 0 reflector) keeps +1
    sgn = self.sign(self.diagonal(rh))
    sgn = self._binary(_lib.OP_ADD, sgn, self._binary(_lib.OP_SUB, 1.0, self.abs(sgn)))
    qh = self._binary(_lib.OP_MUL, qh, sgn)
    rh = self._binary(_lib.OP_MUL, self.reshape(sgn, (sgn.shape[0], 1)), rh)

    def extract(x, rows, cols):
      # complex[i, j] = x[2i, 2j] + i x[2i+1, 2j]  ->  real (rows, cols, 2) gather, viewed as complex
      ld = x.shape[1]
      out = DeviceTensor.empty((rows, cols), mat.code)
      _lib.check(self.lib.tnh_strided_copy(_vp(out), _vp(x), 3, _lib.i64_array((rows, cols, 2)),
                                           _lib.i64_array((2 * ld, 2, ld)), 0, 4 if real == _lib.F32 else 8),
                 "tnh_strided_copy")
      return out

    return extract(qh, m, k), extract(rh, k, n)

  def _qr_prepare(self, tensor, pivot_axis, what):
    tensor = self._as_tensor(tensor)
    self._check_float(tensor, what)
    left_dims = tensor.shape[:pivot_axis]
    right_dims = tensor.shape[pivot_axis:]
    work_code = tensor.code if tensor.code in (_lib.F32, _lib.F64, _lib.C64, _lib.C128) else _lib.F32
    mat = self.cast(tensor, work_code).view((_prod(left_dims), _prod(right_dims)))
    return tensor.code, mat, left_dims, right_dims

  def _phase_fix(self, q, r):
    # decompositions.py:92-95: phases = sign(diag(r)); q = q * phases; r = phases[:, None] * r
    phases = self.sign(self.diagonal(r))
    q = self._binary(_lib.OP_MUL, q, phases)
    r = self._binary(_lib.OP_MUL, self.reshape(self.conj(phases), (phases.shape[0], 1)), r)
    return q, r

  def qr(self, tensor, pivot_axis=-1, non_negative_diagonal=False):
    """QR decomposition (abstract_backend.py:139-145; rule of decompositions.py:77-99):
    reshape to (prod(left), prod(right)) at pivot_axis, thin Householder QR on the GPU
    (tnh_qr: LAPACK's reflector convention, so R has np.linalg.qr's signs), optional
    non-negative-diagonal phase fix, reshape back."""
    orig, mat, left_dims, right_dims = self._qr_prepare(tensor, pivot_axis, "qr")
    q, r = self._qr_matrix(mat)
    if non_negative_diagonal:
      q, r = self._phase_fix(q, r)
    if orig != mat.code:
      q, r = self.cast(q, orig), self.cast(r, orig)
    center = q.shape[1]
    return q.view(tuple(left_dims) + (center,)), r.view((center,) + tuple(right_dims))

  def rq(self, tensor, pivot_axis=-1, non_negative_diagonal=False):
    """RQ decomposition (abstract_backend.py:147-153; decompositions.py:102-124): QR of
    the transposed matrix, phases fixed on that factorisation, then both factors
    transposed back -- M = r q with q's rows orthonormal."""
    orig, mat, left_dims, right_dims = self._qr_prepare(tensor, pivot_axis, "rq")
    q, r = self._qr_matrix(self.conj(self.transpose(mat, (1, 0))))
    if non_negative_diagonal:
      q, r = self._phase_fix(q, r)
    r, q = self.conj(self.transpose(r, (1, 0))), self.conj(self.transpose(q, (1, 0)))
    if orig != mat.code:
      q, r = self.cast(q, orig), self.cast(r, orig)
    center = r.shape[1]
    return r.view(tuple(left_dims) + (center,)), q.view((center,) + tuple(right_dims))

  def eigh(self, matrix):
    """Eigen-decomposition of a real symmetric matrix (abstract_backend.py:320-330; oracle
    np.linalg.eigh): ascending eigenvalues w and eigenvectors as columns of v.

    Runs on the Jacobi SVD kernels: B = A + sigma I with sigma = ||A||_F >= rho(A) is positive
    semi-definite, so its right singular vectors are eigenvectors of A and its singular
    values are lambda + sigma (no +/-lambda mixing, which a plain SVD of an indefinite A
    would suffer).  The eigenvalues are then re-evaluated as Rayleigh quotients
    v_i^T A v_i (one GEMM), which removes the O(sigma eps) shift error to second order."""
    matrix = self._as_tensor(matrix)
    self._check_float(matrix, "eigh")
    if matrix.ndim != 2 or matrix.shape[0] != matrix.shape[1]:
      raise ValueError("Last 2 dimensions of the array must be square")
    n = matrix.shape[0]
    orig = matrix.code
    work_code = orig if orig in (_lib.F32, _lib.F64, _lib.C64, _lib.C128) else _lib.F32
    a = self.cast(matrix, work_code)
    if n == 0:
      return DeviceTensor.empty((0,), orig), DeviceTensor.empty((0, 0), orig)
    # symmetrise from the lower triangle semantics of LAPACK 'L': use (A + A^T) / 2, identical
    # for symmetric input
    a = self._binary(_lib.OP_MUL, self._binary(_lib.OP_ADD, a, self.conj(self.transpose(a, (1, 0)))), 0.5)
    sigma = float(np.real(self.norm(a).item()))
    b = self._binary(_lib.OP_ADD, a, self._binary(_lib.OP_MUL, self.eye(n, dtype=public_dtype(work_code)), sigma))
    _, _, vh, _ = self.svd(b, pivot_axis=1)
    # B = V diag(s) V^H: the rows of vh are conj(eigenvectors); ascending order = reversed rows
    v = self.conj(self.transpose(self.getitem(vh, (slice(None, None, -1), slice(None))), (1, 0)))
    av = self.tensordot(a, v, 1)
    w = self.sum(self._binary(_lib.OP_MUL, self.conj(v), av), axis=(0,))
    if work_code in _REAL_OF:
      w = self._unary(_lib.OP_REAL, w)       # eigenvalues of a Hermitian matrix are real (np.linalg.eigh)
    if orig != work_code:
      w, v = self.cast(w, orig), self.cast(v, orig)
    return w, v

  def inv(self, matrix):
    """Matrix inverse (numpy_backend.py:554-558) through the Jacobi SVD:
    A^-1 = V diag(1/s) U^T."""
    matrix = self._as_tensor(matrix)
    if len(matrix.shape) > 2:
      raise ValueError("input to hip backend method `inv` has shape {}."
                       " Only matrices are supported.".format(matrix.shape))
    if matrix.ndim != 2 or matrix.shape[0] != matrix.shape[1]:
      raise ValueError("Last 2 dimensions of the array must be square")
    u, s, vh, _ = self.svd(matrix, pivot_axis=1)
    # A^-1 = V diag(1/s) U^H  with V = vh^H
    return self.tensordot(self.conj(vh), self.conj(self._binary(_lib.OP_DIV, u, s)), [[0], [1]])

  def expm(self, matrix):
    """Matrix exponential (numpy_backend.py:589-599) as GEMMs only: scaling and squaring
    around a Taylor polynomial in Horner form, ||A / 2^s||_F <= 1/2, degree 18 (f64) /
    10 (f32) -- remainder below the dtype's epsilon."""
    matrix = self._as_tensor(matrix)
    if len(matrix.shape) != 2:
      raise ValueError("input to hip backend method `expm` has shape {}."
                       " Only matrices are supported.".format(matrix.shape))
    if matrix.shape[0] != matrix.shape[1]:
      raise ValueError("input to hip backend method `expm` only supports"
                       " N*N matrix, {x}*{y} matrix is given".format(
                           x=matrix.shape[0], y=matrix.shape[1]))
    self._check_float(matrix, "expm")
    n = matrix.shape[0]
    orig = matrix.code
    work_code = orig if orig not in _HALF else _lib.F32
    a = self.cast(matrix, work_code)
    nrm = float(np.real(self.norm(a).item()))
    squarings = 0 if not np.isfinite(nrm) or nrm <= 0.5 else int(np.ceil(np.log2(nrm))) + 1
    x = self._binary(_lib.OP_MUL, a, 2.0 ** -squarings)
    degree = 18 if work_code in (_lib.F64, _lib.C128) else 10
    eye = self.eye(n, dtype=public_dtype(work_code))
    p = self._binary(_lib.OP_ADD, eye, self._binary(_lib.OP_MUL, x, 1.0 / degree))
    for j in range(degree - 1, 0, -1):
      p = self._binary(_lib.OP_ADD, eye, self._binary(_lib.OP_MUL, self.tensordot(x, p, 1), 1.0 / j))
    for _ in range(squarings):
      p = self.tensordot(p, p, 1)
    return self.cast(p, orig) if orig != work_code else p

  # ------------------------------------------------------------- masks / select
  def is_tensor(self, x):
    return isinstance(x, DeviceTensor)

  def compare(self, op, tensor, other):
    """int32 0/1 mask of ``tensor <op> other`` (op in '<', '<=', '>', '>=', '==', '!='); `other`
    is a real scalar or a tensor of the same shape.  Backs DeviceTensor's comparison operators."""
    ops = {"<": 0, "<=": 1, ">": 2, ">=": 3, "==": 4, "!=": 5}
    tensor = self._as_tensor(tensor)
    if tensor.code in _INT_CODES:
      # integers (and the narrow / unsigned / bool aliases, at their NumPy value) are compared as float64: exact up to
      # 2^53, which covers every integer a tensor network's bookkeeping produces
      tensor = self.cast(tensor, _lib.F64)
    if tensor.code not in (_lib.F32, _lib.F64, _lib.BF16, _lib.F16):
      raise NotImplementedError(f"comparison is not implemented for dtype {tensor.dtype} on the hip backend")
    out = DeviceTensor.empty(tensor.shape, _lib.I32)
    if self._is_scalar(other):
      _lib.check(self.lib.tnh_compare(ops[op], _vp(out), _vp(tensor), None, float(other), tensor.size,
                                      tensor.code), "tnh_compare")
      return out
    other = self.cast(self._as_tensor(other), tensor.code)
    if other.shape != tensor.shape:
      other = self._broadcast_to(other, tensor.shape)
    _lib.check(self.lib.tnh_compare(ops[op], _vp(out), _vp(tensor), _vp(other), 0.0, tensor.size,
                                    tensor.code), "tnh_compare")
    return out

  def index_update(self, tensor, mask, assignee):
    """``t = copy(tensor); t[mask] = assignee`` (abstract_backend.py:685-696; numpy_backend.py:548-552) for a mask
    produced by a tensor comparison (or any array of the tensor's shape).  A scalar (or one-element) assignee fills
    the set positions (the form infinite_mps.py:237-241 uses); a tensor assignee is NumPy's boolean-mask assignment:
    its elements, in row-major order, go to the set positions in row-major order, and their number must match
    (``ValueError`` as NumPy raises it) -- compacted on the device (``tnh_masked_scatter``)."""
    tensor = self._as_tensor(tensor)
    self._check_float(tensor, "index_update")
    if isinstance(assignee, DeviceTensor) and assignee.size == 1:
      assignee = assignee.item()
    elif isinstance(assignee, np.ndarray) and assignee.size == 1:
      assignee = assignee.reshape(()).item()
    if not self._is_scalar(assignee):
      return self._index_update_tensor(tensor, mask, assignee)
    if not isinstance(mask, DeviceTensor):
      mask = DeviceTensor.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.int32))
    elif mask.code != _lib.I32:
      mask = self.compare("!=", mask, 0.0)
    if mask.shape != tensor.shape:
      raise ValueError(f"mask shape {mask.shape} does not match tensor shape {tensor.shape}")
    value = complex(assignee)
    if value.imag != 0.0 and not tensor.is_complex:
      raise TypeError("cannot assign a complex value into a real tensor")
    out = DeviceTensor.empty(tensor.shape, tensor.code)
    _lib.check(self.lib.tnh_masked_fill(_vp(out), _vp(tensor), _vp(mask), value.real, value.imag, tensor.size,
                                        tensor.code), "tnh_masked_fill")
    return out

  def _index_update_tensor(self, tensor, mask, assignee):
    values = self._as_tensor(assignee)
    if values.is_complex and not tensor.is_complex:
      raise TypeError("cannot assign complex values into a real tensor")
    values = self.cast(values, tensor.code)
    if not isinstance(mask, DeviceTensor):
      mask = DeviceTensor.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.int32))
    elif mask.code != _lib.I32:
      mask = self.compare("!=", mask, 0.0)
    if mask.shape != tensor.shape:
      raise ValueError(f"mask shape {mask.shape} does not match tensor shape {tensor.shape}")
    out = DeviceTensor.empty(tensor.shape, tensor.code, tensor.alias)
    count = ctypes.c_int64(0)
    _lib.check(self.lib.tnh_masked_scatter(_vp(out), _vp(tensor), _vp(mask), _vp(values), values.size, tensor.size,
                                           tensor.itemsize, ctypes.byref(count)), "tnh_masked_scatter")
    if count.value != values.size:
      raise ValueError(f"NumPy boolean array indexing assignment cannot assign {values.size} input values to "
                       f"the {count.value} output values where the mask is true")
    return out

  # ------------------------------------------------------------------ Krylov
  def eigsh_lanczos(self, A, args=None, initial_state=None, shape=None, dtype=None, num_krylov_vecs=20,
                    numeig=1, tol=1E-8, delta=1E-8, ndiag=20, reorthogonalize=False):
    """Lanczos on device vectors (abstract_backend.py:428-476; algorithm of
    numpy_backend.py:415-534) -- see tensornetwork_amd/krylov.py."""
    from tensornetwork_amd import krylov  # pylint: disable=import-outside-toplevel
    if initial_state is not None and not isinstance(initial_state, DeviceTensor):
      raise TypeError("Expected a `DeviceTensor`. Got {}".format(type(initial_state)))
    return krylov.eigsh_lanczos(self, A, args, initial_state, shape, dtype, num_krylov_vecs, numeig, tol,
                                delta, ndiag, reorthogonalize)

  def eigsh(self, A, args=None, initial_state=None, shape=None, dtype=None, num_krylov_vecs=50, numeig=1,
            tol=1E-8, which='LR', maxiter=None):
    """Thick-restart Lanczos on device vectors.  Signature and defaults of the interface
    (abstract_backend.py:380-426; the reference's NumPy backend declares the same signature and raises
    NotImplementedError, numpy_backend.py:168-214).  For a Hermitian operator the interface's 'LR' / 'SR' (largest /
    smallest real part) are scipy's 'LA' / 'SA', which are accepted too."""
    from tensornetwork_amd import krylov  # pylint: disable=import-outside-toplevel
    which = {'LR': 'LA', 'SR': 'SA'}.get(which, which)
    if initial_state is not None and not isinstance(initial_state, DeviceTensor):
      raise TypeError("Expected a `DeviceTensor`. Got {}".format(type(initial_state)))
    return krylov.eigsh(self, A, args, initial_state, shape, dtype, num_krylov_vecs, numeig, tol, which, maxiter)

  def eigs(self, A, args=None, initial_state=None, shape=None, dtype=None, num_krylov_vecs=50, numeig=6,
           tol=1E-8, which='LR', maxiter=None):
    """Krylov-Schur restarted Arnoldi on device vectors (abstract_backend.py:331-378; the reference
    wraps scipy.sparse.linalg.eigs, numpy_backend.py:216-283)."""
    from tensornetwork_amd import krylov  # pylint: disable=import-outside-toplevel
    if initial_state is not None and not isinstance(initial_state, DeviceTensor):
      raise TypeError("Expected a `DeviceTensor`. Got {}".format(type(initial_state)))
    return krylov.eigs(self, A, args, initial_state, shape, dtype, num_krylov_vecs, numeig, tol, which, maxiter)

  def gmres(self, A_mv, b, A_args=None, A_kwargs=None, x0=None, tol=1E-05, atol=None,
            num_krylov_vectors=20, maxiter=1, M=None):
    """GMRES on device vectors; argument checks of abstract_backend.py:560-616, solver in
    tensornetwork_amd/krylov.py (the reference wraps scipy.sparse.linalg.gmres)."""
    from tensornetwork_amd import krylov  # pylint: disable=import-outside-toplevel
    b = self._as_tensor(b)
    bshape = self.shape_tensor(b)
    N = int(self.shape_prod(bshape)) if bshape else 1
    dtype = b.dtype
    if x0 is None:
      x0 = self.zeros((N,), dtype)
    else:
      x0 = self._as_tensor(x0)
      x0shape = self.shape_tensor(x0)
      if x0shape != bshape:
        raise ValueError(f"If x0 is supplied, its shape, {x0shape}, must match b's, {bshape}.")
      if x0.dtype != dtype:
        raise TypeError(f"If x0 is supplied, its dtype, {x0.dtype}, must match b's, {dtype}.")
      x0 = self.reshape(x0, (N,))
    if num_krylov_vectors > N:
      num_krylov_vectors = N
    if tol < 0:
      raise ValueError(f"tol = {tol} must be positive.")
    if atol is None:
      atol = tol
    elif atol < 0:
      raise ValueError(f"atol = {atol} must be positive.")
    if num_krylov_vectors <= 0:
      raise ValueError(f"num_krylov_vectors must be positive, not{num_krylov_vectors}.")
    if A_args is None:
      A_args = []
    if A_kwargs is None:
      A_kwargs = {}
    return krylov.gmres(self, A_mv, b, A_args, A_kwargs, x0, tol, atol, num_krylov_vectors, maxiter, M=M)

  def _gmres(self, A_mv, b, A_args, A_kwargs, x0, tol, atol, num_krylov_vectors, maxiter, M=None):
    """The solver behind `gmres` after argument checks (abstract_backend.py:618-631)."""
    from tensornetwork_amd import krylov  # pylint: disable=import-outside-toplevel
    return krylov.gmres(self, A_mv, b, A_args, A_kwargs, x0, tol, atol, num_krylov_vectors, maxiter, M=M)

  def pivot(self, tensor, pivot_axis=-1):
    """Tensor -> matrix about `pivot_axis` (abstract_backend.py:938-962): a view, no data movement."""
    tensor = self._as_tensor(tensor)
    ndim = len(tensor.shape)
    if pivot_axis > ndim:
      raise ValueError(f"pivot_axis = {pivot_axis} was invalid given ndim={ndim} array.")
    left, right = tensor.shape[:pivot_axis], tensor.shape[pivot_axis:]
    return self.reshape(tensor, [int(np.prod(left, dtype=np.int64)), int(np.prod(right, dtype=np.int64))])

  def cholesky(self, tensor, pivot_axis=-1, non_negative_diagonal=False):
    # abstract_backend.py:1026-1032: no reference backend implements cholesky either.
    raise NotImplementedError(f"Backend {self.name} has not implemented cholesky.")

  # ------------------------------------------------------------------- misc
  def jit(self, fun, *args, **kwargs):  # pylint: disable=unused-argument
    return fun

  def item(self, tensor):
    return self._as_tensor(tensor).item()

  def eps(self, dtype):
    if dtype is bfloat16:
      return 2.0**-7
    return np.finfo(dtype).eps

  def serialize_tensor(self, tensor):
    # wire format of numpy_backend.py:732-744 (np.save bytes as latin-1 str)
    m = io.BytesIO()
    np.save(m, self._as_tensor(tensor).numpy(), allow_pickle=False)
    m.seek(0)
    return str(m.read(), encoding='latin-1')

  def deserialize_tensor(self, s):
    m = io.BytesIO()
    m.write(s.encode('latin-1'))
    m.seek(0)
    return self.convert_to_tensor(np.load(m))


class DeviceGraph:
  """An instantiated hipGraph of one launch sequence plus the HBM arena it runs in
  (``tnh_graph_*`` in include/tnh.h).  Every block the sequence touched stays pinned to
  the graph until it is destroyed, so replays cannot collide with other tensors."""

  def __init__(self, backend, fun, args):
    self._lib = backend.lib
    self._exec = None
    self._args = args            # keep the captured input blocks alive
    _lib.check(self._lib.tnh_graph_begin(), "tnh_graph_begin")
    handle = ctypes.c_void_p()
    try:
      self.outputs = fun(*args)
    except BaseException:
      if self._lib.tnh_graph_end(ctypes.byref(handle)) == 0 and handle:
        self._lib.tnh_graph_destroy(handle)
      raise
    _lib.check(self._lib.tnh_graph_end(ctypes.byref(handle)), "tnh_graph_end")
    self._exec = handle

  def launch(self):
    _lib.check(self._lib.tnh_graph_launch(self._exec), "tnh_graph_launch")
    return self.outputs

  def close(self):
    if self._exec is not None:
      self._lib.tnh_graph_destroy(self._exec)
      self._exec = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass


_BACKEND = None


def get_hip_backend():
  """Process-wide singleton (backends are singletons per name, factory:42-46)."""
  global _BACKEND
  if _BACKEND is None:
    _BACKEND = HipBackend()
  return _BACKEND


def register_with_tensornetwork():
  """Insert ``"hip"`` into tensornetwork's backend registry (factory:22-28).

  Needed because ``contract`` / Node arithmetic rebuild nodes from
  ``backend.name`` (network_components.py:1879-1882) and
  ``set_default_backend`` validates names (backend_contextmanager.py:47-48).
  """
  if not HAVE_TENSORNETWORK:
    return False
  from tensornetwork.backends import backend_factory  # pylint: disable=import-outside-toplevel
  backend_factory._BACKENDS["hip"] = HipBackend  # pylint: disable=protected-access
  backend_factory._INSTANTIATED_BACKENDS["hip"] = get_hip_backend()  # pylint: disable=protected-access
  return True
