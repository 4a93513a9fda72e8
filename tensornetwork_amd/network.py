"""Minimal Node/Edge graph layer over an ``AbstractBackend``-shaped backend.

On a machine with google/TensorNetwork installed, use its own ``tn.Node`` with
``backend="hip"`` -- the hip backend is a drop-in there.  This module exists so
that the same workloads (``contract_between``, ``split_node``, the contractors)
run stand-alone on a GPU box that only has this repository; it mirrors the
reference's public behaviour for exactly those entry points:

  * ``contract_between``  -- ``network_components.py:1984-2095``
  * ``contract`` (one edge), trace edges -- ``:1834-1885``, ``:1802-1831``
  * ``outer_product``     -- ``:2127-2186``
  * ``split_node`` / ``split_node_full_svd`` -- ``network_operations.py:130-255, 446-588``
  * ``copy`` / ``slice_edge`` -- ``network_operations.py:32-83``, ``network_components.py:1636-1682``

All tensor math goes through ``node.backend``.
"""
from typing import Any, Dict, Iterable, List, Optional, Sequence, Set, Tuple

import math

import numpy as np


_rb = None


def _resolve_backend(backend):
  global _rb  # pylint: disable=global-statement
  if _rb is None:
    from tensornetwork_amd.ncon import _resolve_backend as _rb_  # pylint: disable=import-outside-toplevel
    _rb = _rb_
  return _rb(backend)


_AXIS_NAMES = tuple(str(i) for i in range(64))      # default axis names "0", "1", ...


class NodeCollection:
  """`with NodeCollection(container):` -- every node created inside the block is added to `container`
  (a list or a set); nested blocks collect into the innermost one (network_components.py:2189-2240)."""
  _stack: List["NodeCollection"] = []

  def __init__(self, container):
    if not isinstance(container, (list, set)):
      raise ValueError("Item passed to NodeCollection must be list or set")
    self._container = container

  def add(self, node) -> None:
    if isinstance(self._container, set):
      self._container.add(node)
    else:
      self._container.append(node)

  def __enter__(self):
    NodeCollection._stack.append(self)

  def __exit__(self, exc_type, exc_val, exc_tb):
    NodeCollection._stack.pop()

  @classmethod
  def _register(cls, node) -> None:
    if cls._stack:
      cls._stack[-1].add(node)


class Edge:
  """A (possibly dangling) connection between one or two node axes."""

  def __init__(self, node1: "Node", axis1: int, name: Optional[str] = None,
               node2: Optional["Node"] = None, axis2: Optional[int] = None):
    self.node1, self.axis1 = node1, axis1
    self.node2, self.axis2 = node2, axis2
    self.name = name if name is not None else "__unnamed_edge__"

  def is_dangling(self) -> bool:
    return self.node2 is None

  def is_trace(self) -> bool:
    return self.node1 is self.node2

  @property
  def dimension(self) -> int:
    return self.node1.shape[self.axis1]

  def get_nodes(self):
    return [self.node1, self.node2]

  def ends(self):
    out = [(self.node1, self.axis1)]
    if self.node2 is not None:
      out.append((self.node2, self.axis2))
    return out

  def _retarget(self, old_node, old_axis, new_node, new_axis):
    """Point the end (old_node, old_axis) at (new_node, new_axis)."""
    if self.node1 is old_node and self.axis1 == old_axis:
      self.node1, self.axis1 = new_node, new_axis
    elif self.node2 is old_node and self.axis2 == old_axis:
      self.node2, self.axis2 = new_node, new_axis
    else:
      raise ValueError("edge end not found")

  def update_axis(self, old_axis: int, old_node: "Node", new_axis: int, new_node: "Node") -> None:
    """Repoint the end (old_node, old_axis) to (new_node, new_axis) (network_components.py:1075-1094)."""
    try:
      self._retarget(old_node, old_axis, new_node, new_axis)
    except ValueError as err:
      raise ValueError("Edge '{}' did not contain node '{}' on axis {}. node1: '{}', axis1: {}, node2: '{}', "
                       "axis2: {}".format(self, old_node, old_axis, self.node1, self.axis1, self.node2,
                                          self.axis2)) from err

  def is_being_used(self) -> bool:
    """True while the edge still sits in an edge slot of one of its nodes."""
    return any(n is not None and any(e is self for e in n.edges) for n in (self.node1, self.node2))

  def set_name(self, name: str) -> None:
    if not isinstance(name, str):
      raise TypeError("Edge name should be str type")
    self.name = name

  def disconnect(self, edge1_name: Optional[str] = None, edge2_name: Optional[str] = None):
    return disconnect(self, edge1_name, edge2_name)

  def __or__(self, other: "Edge"):
    """`edge | edge` breaks a connected edge into its two dangling halves (1263-1266)."""
    if other is not self:
      raise ValueError('Cannot break two unconnected edges')
    return self.disconnect()

  def __lt__(self, other) -> bool:
    if not isinstance(other, Edge):
      raise TypeError("Cannot compare 'Edge' with type {}".format(type(other)))
    return id(self) < id(other)

  def __str__(self) -> str:
    return self.name if self.name else '__unnamed_edge__'

  def __xor__(self, other: "Edge") -> "Edge":
    return connect(self, other)

  def __repr__(self):
    return f"Edge({self.name!r}, dim={self.dimension}, dangling={self.is_dangling()})"


class Node:
  """A tensor with one edge per axis."""

  def __init__(self, tensor: Any, name: Optional[str] = None, axis_names: Optional[List[str]] = None,
               backend=None):
    self.backend = _resolve_backend(backend)
    if isinstance(tensor, Node):
      tensor = tensor.tensor
    self.tensor = self.backend.convert_to_tensor(tensor)
    if name is not None and not isinstance(name, str):
      raise TypeError("Node name should be str type")
    if axis_names is not None and any(not isinstance(n, str) for n in axis_names):
      raise TypeError("axis_names should be str type")
    self.name = name if name is not None else "__unnamed_node__"
    rank = len(self.backend.shape_tuple(self.tensor))
    if axis_names is not None and len(axis_names) != rank:
      raise ValueError("axis_names is not the same length as the tensor shape."
                       f"axis_names length: {len(axis_names)}, shape length: {rank}")
    if axis_names is not None:
      self.axis_names = list(axis_names)
    else:
      self.axis_names = list(_AXIS_NAMES[:rank]) if rank <= 64 else [str(i) for i in range(rank)]
    self.edges: List[Edge] = [Edge(self, i, n) for i, n in enumerate(self.axis_names)]
    if NodeCollection._stack:  # pylint: disable=protected-access
      NodeCollection._register(self)  # pylint: disable=protected-access

  @classmethod
  def _from_contraction(cls, tensor, name, backend, sources):
    """The node of a contraction result: `tensor` (already the backend's tensor type) with the live edges that sat on
    the listed (node, axis) slots, in that order -- what ``Node(tensor)`` followed by ``_adopt_edges`` builds, without
    the rank fresh dangling edges that construction makes and drops (a D = 32 contract_between is host-bound)."""
    if name is not None and not isinstance(name, str):
      raise TypeError("Node name should be str type")
    self = cls.__new__(cls)
    self.backend = backend
    self.tensor = tensor
    self.name = name if name is not None else "__unnamed_node__"
    edges, names = [], []
    for new_axis, (old_node, old_axis) in enumerate(sources):
      e = old_node.edges[old_axis]
      e._retarget(old_node, old_axis, self, new_axis)  # pylint: disable=protected-access
      edges.append(e)
      names.append(old_node.axis_names[old_axis])
    self.edges = edges
    self.axis_names = names
    if NodeCollection._stack:  # pylint: disable=protected-access
      NodeCollection._register(self)  # pylint: disable=protected-access
    return self

  @property
  def shape(self) -> Tuple[int, ...]:
    return tuple(self.backend.shape_tuple(self.tensor))

  @property
  def dtype(self):
    return self.tensor.dtype

  def get_rank(self) -> int:
    return len(self.shape)

  def get_all_dangling(self) -> List[Edge]:
    return [e for e in self.edges if e.is_dangling()]

  def get_all_nondangling(self) -> Set[Edge]:
    return {e for e in self.edges if not e.is_dangling()}

  def get_axis_number(self, axis) -> int:
    if isinstance(axis, int):
      return axis
    if axis not in self.axis_names:
      raise ValueError(f"Axis name '{axis}' not found for node '{self.name}'")
    return self.axis_names.index(axis)

  def get_dimension(self, axis) -> int:
    num = self.get_axis_number(axis)
    if num < 0 or num >= len(self.shape):
      raise ValueError("Axis must be positive and less than rank of the tensor")
    return self.shape[num]

  def get_edge(self, key) -> Edge:
    return self.edges[self.get_axis_number(key)]

  def get_all_edges(self) -> List[Edge]:
    return list(self.edges)

  def has_nondangling_edge(self) -> bool:
    return any(not e.is_dangling() for e in self.edges)

  def has_dangling_edge(self) -> bool:
    return any(e.is_dangling() for e in self.edges)

  def set_name(self, name: str) -> None:
    if not isinstance(name, str):
      raise TypeError("Node name should be str type")
    self.name = name

  def add_axis_names(self, axis_names: List[str]) -> None:
    """Name the axes (network_components.py:128-148): unique strings, one per axis."""
    if len(axis_names) != len(set(axis_names)):
      raise ValueError("Not all axis names are unique.")
    if len(axis_names) != len(self.shape):
      raise ValueError("axis_names is not the same length as the tensor shape."
                       "axis_names length: {}, tensor.shape length: {}".format(len(axis_names), len(self.shape)))
    if any(not isinstance(n, str) for n in axis_names):
      raise TypeError("axis_names should be str type")
    self.axis_names = list(axis_names)

  def add_edge(self, edge: Edge, axis, override: bool = False) -> None:
    """Put `edge` into the slot of `axis` (150-173); an occupied (non-dangling) slot needs `override`."""
    num = self.get_axis_number(axis)
    if num < 0 or num >= len(self.shape):
      raise ValueError("Axis must be positive and less than rank of the tensor")
    if not self.edges[num].is_dangling() and not override:
      raise ValueError("Node '{}' already has a non-dangling edge for axis {}".format(self, axis))
    self.edges[num] = edge

  @property
  def sparse_shape(self):
    return self.backend.sparse_shape(self.tensor)

  def copy(self, conjugate: bool = False) -> "Node":
    """A node with the same (optionally conjugated) tensor and names, all edges dangling except its own
    trace edges (network_components.py:637-660)."""
    tensor = self.backend.conj(self.tensor) if conjugate else self.tensor
    new = Node(tensor, name=self.name, axis_names=list(self.axis_names), backend=self.backend)
    for i, e in enumerate(self.edges):
      new.edges[i].name = e.name
      if e.node1 is self and e.node2 is self and i == e.axis1:
        connect(new.edges[e.axis1], new.edges[e.axis2], name=e.name)
    return new

  def __getitem__(self, key):
    if isinstance(key, slice):
      return self.edges[key]
    return self.get_edge(key)

  def __str__(self) -> str:
    return self.name

  def __lt__(self, other) -> bool:
    if not isinstance(other, Node):
      raise ValueError("Object {} is not a Node type.".format(other))
    return id(self) < id(other)

  def reorder_edges(self, edge_order: Sequence[Edge]) -> "Node":
    """Permute the tensor so that its axes follow `edge_order` (network_components.py:212-252)."""
    if set(edge_order) != set(self.edges) or len(edge_order) != len(self.edges):
      raise ValueError("Given edge order does not match expected edges. "
                       f"Found: {edge_order}, Expected: {self.edges}")
    perm = []
    for e in edge_order:
      cands = [i for i, mine in enumerate(self.edges) if mine is e and i not in perm]
      perm.append(cands[0])
    return self.reorder_axes(perm)

  def reorder_axes(self, perm: Sequence[int]) -> "Node":
    perm = list(perm)
    if sorted(perm) != list(range(len(self.edges))):
      raise ValueError(f"Given perm does not match expected axes: {perm}")
    old_edges = list(self.edges)
    self.tensor = self.backend.transpose(self.tensor, tuple(perm))
    self.edges = [old_edges[p] for p in perm]
    self.axis_names = [self.axis_names[p] for p in perm]
    done = set()
    for new_axis, (old_axis, e) in enumerate(zip(perm, self.edges)):
      # an edge may appear twice (trace edge): retarget each end once
      key = (id(e), old_axis)
      if key in done:
        continue
      done.add(key)
      e._retarget(self, old_axis, self, -1 - new_axis)  # park on a temp axis  # pylint: disable=protected-access
    for e in set(self.edges):
      if e.node1 is self and e.axis1 < 0:
        e.axis1 = -1 - e.axis1
      if e.node2 is self and e.axis2 is not None and e.axis2 < 0:
        e.axis2 = -1 - e.axis2
    return self

  def tensor_from_edge_order(self, edge_order: Sequence[Edge]):
    perm = []
    for e in edge_order:
      cands = [i for i, mine in enumerate(self.edges) if mine is e and i not in perm]
      if not cands:
        raise ValueError("edge does not belong to this node")
      perm.append(cands[0])
    if sorted(perm) != list(range(len(self.edges))):
      raise ValueError("edge_order must contain every edge of the node exactly once")
    return self.backend.transpose(self.tensor, tuple(perm))

  def __matmul__(self, other: "Node") -> "Node":
    if not isinstance(other, Node):
      raise TypeError("Cannot use '@' with type '{}'".format(type(other)))
    return contract_between(self, other)

  # Elementwise arithmetic with a scalar or another Node (network_components.py:586-631): the result is a
  # new, unconnected Node carrying this node's name.
  def _operand(self, other):
    if isinstance(other, CopyNode) or isinstance(self, CopyNode):
      raise NotImplementedError("CopyNode does not implement elementwise arithmetic")
    if not isinstance(other, (int, float, complex, Node)):
      raise TypeError("Operand should be one of int, float, Node type")
    if isinstance(other, Node):
      if self.backend.name != other.backend.name:
        raise TypeError("Operands backend must match.\noperand 1 backend: {}\noperand 2 backend: {}"
                        .format(self.backend.name, other.backend.name))
      return other.tensor
    return other

  def __add__(self, other):
    return Node(self.backend.addition(self.tensor, self._operand(other)), name=self.name, backend=self.backend)

  def __sub__(self, other):
    return Node(self.backend.subtraction(self.tensor, self._operand(other)), name=self.name, backend=self.backend)

  def __mul__(self, other):
    return Node(self.backend.multiply(self.tensor, self._operand(other)), name=self.name, backend=self.backend)

  def __truediv__(self, other):
    return Node(self.backend.divide(self.tensor, self._operand(other)), name=self.name, backend=self.backend)

  def get_tensor(self):
    return self.tensor

  def set_tensor(self, tensor) -> None:
    self.tensor = tensor

  def __repr__(self):
    return f"Node(name={self.name!r}, shape={self.shape}, backend={self.backend.name!r})"


class CopyNode(Node):
  """The rank-`rank` "copy" (generalised delta) tensor of leg dimension `dimension`: 1 where all indices
  agree, else 0 (network_components.py:737-935).  The dense tensor is only built if somebody asks for
  `.tensor`; `contract_copy_node` contracts it with ALL its neighbours as one hyper-index einsum instead."""

  def __init__(self, rank: int, dimension: int, name: Optional[str] = None,
               axis_names: Optional[List[str]] = None, backend=None, dtype=np.float64):
    # pylint: disable=super-init-not-called
    self.backend = _resolve_backend(backend)
    self.rank, self.dimension, self.copy_node_dtype = rank, dimension, dtype
    self._dense = None
    self.name = name if name is not None else "__unnamed_node__"
    if axis_names is not None and len(axis_names) != rank:
      raise ValueError("axis_names is not the same length as the tensor shape."
                       f"axis_names length: {len(axis_names)}, shape length: {rank}")
    self.axis_names = list(axis_names) if axis_names is not None else [str(i) for i in range(rank)]
    self.edges = [Edge(self, i, name=self.axis_names[i]) for i in range(rank)]
    NodeCollection._register(self)  # pylint: disable=protected-access

  @staticmethod
  def make_copy_tensor(rank: int, dimension: int, dtype) -> np.ndarray:
    out = np.zeros((dimension,) * rank, dtype=dtype)
    idx = np.arange(dimension)
    out[(idx,) * rank] = 1
    return out

  @property
  def tensor(self):
    if self._dense is None:
      self._dense = self.backend.convert_to_tensor(
          self.make_copy_tensor(self.rank, self.dimension, self.copy_node_dtype))
    return self._dense

  @tensor.setter
  def tensor(self, value):
    self._dense = value

  @property
  def shape(self) -> Tuple[int, ...]:
    return (self.dimension,) * self.rank

  @property
  def dtype(self):
    return self.copy_node_dtype        # without building the dense tensor

  def get_partners(self) -> Dict[Node, Set[int]]:
    """{neighbour: axes of the neighbour that connect to this copy node} (trace edges of the copy
    node itself are skipped; a dangling leg is an error)."""
    partners: Dict[Node, Set[int]] = {}
    for e in self.edges:
      if e.is_dangling():
        raise ValueError('Cannot contract copy tensor with dangling edges')
      if e.node1 is self and e.node2 is self:
        continue
      other, axis = (e.node2, e.axis2) if e.node1 is self else (e.node1, e.axis1)
      partners.setdefault(other, set()).add(axis)
    return partners

  def compute_contracted_tensor(self):
    """einsum of all neighbours with ONE shared index in place of the copy tensor; free axes in
    neighbour order (network_components.py:875-909)."""
    from tensornetwork_amd.ncon import einsum as _einsum  # pylint: disable=import-outside-toplevel
    letters = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'
    partners = self.get_partners()
    nxt, terms = 1, []
    for node, shared in partners.items():
      term = ""
      for axis in range(node.get_rank()):
        if axis in shared:
          term += letters[0]
        else:
          term += letters[nxt]
          nxt += 1
      terms.append(term)
    expr = ",".join(terms) + "->" + letters[1:nxt]
    return _einsum(expr, *[n.tensor for n in partners], backend=self.backend)


# ---------------------------------------------------------------------- wiring
def connect(edge1: Edge, edge2: Edge, name: Optional[str] = None) -> Edge:
  """Join two dangling edges (network_components.py:1939-1981)."""
  if edge1 is edge2:
    raise ValueError(f"Cannot connect edge '{edge1}' to itself.")
  for e in (edge1, edge2):
    if not e.is_dangling():
      raise ValueError(f"Edge '{e}' is not a dangling edge. This edge points to nodes: "
                       f"'{e.node1}' and '{e.node2}'")
  if edge1.dimension != edge2.dimension:
    raise ValueError(f"Cannot connect edges of unequal dimension. Dimension of edge '{edge1}': "
                     f"{edge1.dimension}, Dimension of edge '{edge2}': {edge2.dimension}.")
  n1, a1, n2, a2 = edge1.node1, edge1.axis1, edge2.node1, edge2.axis1
  new = Edge(n1, a1, name=name, node2=n2, axis2=a2)
  n1.edges[a1] = new
  n2.edges[a2] = new
  return new


def get_shared_edges(node1: Node, node2: Node) -> Set[Edge]:
  """Edges whose two ends are exactly {node1, node2} (network_components.py:1278-1299); for
  node1 is node2 these are the node's trace edges."""
  out = set()
  for e in node1.edges:
    x, y = e.node1, e.node2
    if y is not None and ((x is node1 and y is node2) or (x is node2 and y is node1)):
      out.add(e)
  return out


def get_all_edges(nodes: Iterable[Node]) -> Set[Edge]:
  return {e for n in nodes for e in n.edges}


def get_subgraph_dangling(nodes: Iterable[Node]) -> Set[Edge]:
  nodes = list(nodes)
  inside = set(map(id, nodes))
  out = set()
  for n in nodes:
    for e in n.edges:
      if e.is_dangling() or not all(id(x) in inside for x in e.get_nodes()):
        out.add(e)
  return out


def reachable(node: Node) -> Set[Node]:
  seen, stack = {id(node): node}, [node]
  while stack:
    cur = stack.pop()
    for e in cur.edges:
      for nb in e.get_nodes():
        if nb is not None and id(nb) not in seen:
          seen[id(nb)] = nb
          stack.append(nb)
  return set(seen.values())


def _adopt_edges(new_node: Node, sources: Sequence[Tuple[Node, int]]):
  """Give `new_node` the (still live) edges that sat on the listed (node, axis) slots."""
  for new_axis, (old_node, old_axis) in enumerate(sources):
    e = old_node.edges[old_axis]
    e._retarget(old_node, old_axis, new_node, new_axis)  # pylint: disable=protected-access
    new_node.edges[new_axis] = e
    new_node.axis_names[new_axis] = old_node.axis_names[old_axis]


# ------------------------------------------------------------------ contraction
def contract_trace_edges(node: Node) -> Node:
  """Contract every trace edge of `node` (network_operations.py:737-751)."""
  trace_edges = []
  for e in node.edges:
    if e.is_trace() and e not in trace_edges:
      trace_edges.append(e)
  if not trace_edges:
    return node
  be = node.backend
  first = [e.axis1 for e in trace_edges]
  second = [e.axis2 for e in trace_edges]
  free = [i for i in range(len(node.edges)) if i not in first + second]
  shape = node.shape
  cdim = math.prod(int(shape[i]) for i in first)
  t = be.transpose(node.tensor, tuple(free + first + second))
  t = be.reshape(t, tuple(shape[i] for i in free) + (cdim, cdim))
  out = Node(be.trace(t), name=node.name, backend=be)
  _adopt_edges(out, [(node, i) for i in free])
  return out


def contract(edge: Edge, name: Optional[str] = None) -> Node:
  """Contract a single edge (network_components.py:1834-1885)."""
  if edge.is_dangling():
    raise ValueError(f"Attempting to contract dangling edge '{edge}'")
  if edge.is_trace():
    node = edge.node1
    be = node.backend
    a1, a2 = edge.axis1, edge.axis2
    free = [i for i in range(len(node.edges)) if i not in (a1, a2)]
    t = be.trace(be.transpose(node.tensor, tuple(free + [a1, a2])))
    out = Node(t, name=name, backend=be)
    _adopt_edges(out, [(node, i) for i in free])
    return out
  n1, n2 = edge.node1, edge.node2
  be = n1.backend
  t = be.tensordot(n1.tensor, n2.tensor, [[edge.axis1], [edge.axis2]])
  out = Node(t, name=name, backend=be)
  sources = [(n1, i) for i in range(len(n1.edges)) if i != edge.axis1] + \
            [(n2, i) for i in range(len(n2.edges)) if i != edge.axis2]
  _adopt_edges(out, sources)
  return out


def outer_product(node1: Node, node2: Node, name: Optional[str] = None) -> Node:
  """Tensor product of two nodes (network_components.py:2127-2186)."""
  be = node1.backend
  if node1.get_rank() == 0 or node2.get_rank() == 0:
    t = be.multiply(node1.tensor, node2.tensor)
  else:
    t = be.outer_product(node1.tensor, node2.tensor)
  out = Node(t, name=name, backend=be)
  _adopt_edges(out, [(node1, i) for i in range(len(node1.edges))] +
               [(node2, i) for i in range(len(node2.edges))])
  return out


def outer_product_final_nodes(nodes: Iterable[Node], edge_order: List[Edge]) -> Node:
  """Outer product of fully contracted (all edges dangling) nodes, axes in `edge_order`
  (network_components.py:2098-2124)."""
  nodes = list(nodes)
  for node in nodes:
    if node.has_nondangling_edge():
      raise ValueError("Node '{}' has a non-dangling edge remaining.".format(node))
  final = nodes[0]
  for node in nodes[1:]:
    final = outer_product(final, node)
  return final.reorder_edges(list(edge_order))


def contract_between(node1: Node, node2: Node, name: Optional[str] = None,
                     allow_outer_product: bool = False,
                     output_edge_order: Optional[Sequence[Edge]] = None,
                     axis_names: Optional[List[str]] = None,
                     edge_time: Optional[Dict[Edge, int]] = None) -> Node:
  """Contract all edges shared by two nodes with ONE tensordot
  (network_components.py:1984-2095).

  ``edge_time`` (from a contractor that knows the whole path: edge -> index of the step that
  contracts it) turns on layout planning when the backend offers ``tensordot_planned``: the
  operand whose legs are contracted soonest goes second, and the free axes of an operand are
  requested latest-first / soonest-last, so that the legs of the NEXT contractions end up trailing
  in the result -- the K-contiguous form the GEMM consumes without another permute.  The axis order
  of an intermediate is bookkeeping here (edges follow their axes), so this is free to choose."""
  if node1.backend.name != node2.backend.name:
    raise ValueError(f"The backends of {node1} and {node2} do not match: "
                     f"{node1.backend.name} vs {node2.backend.name}")
  be = node1.backend
  if node1 is node2:
    out = contract_trace_edges(node1)
    out.name = name if name is not None else out.name
    if output_edge_order is not None:
      out.reorder_edges(list(output_edge_order))
    return out
  shared = get_shared_edges(node1, node2)
  if not shared:
    if not allow_outer_product:
      raise ValueError(f"No edges found between nodes '{node1}' and '{node2}' and "
                       "allow_outer_product=False.")
    out = outer_product(node1, node2, name=name)
  else:
    # (axis on node1, axis on node2) per shared edge, sorted by node1's axis so the
    # contracted group is traversed in node1's memory order.
    pairs = []
    for e in shared:
      if e.node1 is node1:
        pairs.append((e.axis1, e.axis2))
      else:
        pairs.append((e.axis2, e.axis1))
    pairs.sort()
    axes1, axes2 = [p[0] for p in pairs], [p[1] for p in pairs]
    if edge_time is not None and output_edge_order is None and hasattr(be, "tensordot_planned"):
      never = float("inf")

      def plan(node, axes):
        free = [i for i in range(len(node.edges)) if i not in axes]
        when = {i: edge_time.get(node.edges[i], never) for i in free}
        order = sorted(free, key=lambda i: -when[i] if when[i] != never else float("-inf"))
        return order, min(when.values(), default=never)

      order1, soon1 = plan(node1, axes1)
      order2, soon2 = plan(node2, axes2)
      if soon1 < soon2:   # node1's legs are needed first: it goes second so that they end up trailing
        node1, node2, axes1, axes2, order1, order2 = node2, node1, axes2, axes1, order2, order1
        pairs = sorted(zip(axes1, axes2))
        axes1, axes2 = [p[0] for p in pairs], [p[1] for p in pairs]
      # Where the gather GEMM can write the result in any order for free (tnh_gemm_gather_scatter, runs of at least
      # `gather_scatter_min_run_bytes`: profiles/gather_scatter.md) ask for ALL remaining legs latest-contracted first,
      # interleaved across both operands, instead of one order per operand.
      min_run = getattr(be, "gather_scatter_min_run_bytes", None)
      order = None
      if min_run is not None and hasattr(be, "scatter_run_bytes"):
        legs = [(node1, i) for i in range(len(node1.edges)) if i not in axes1] + \
               [(node2, i) for i in range(len(node2.edges)) if i not in axes2]
        when = [edge_time.get(n.edges[i], never) for n, i in legs]
        order = sorted(range(len(legs)), key=lambda p: -when[p] if when[p] != never else float("-inf"))
        if order == list(range(len(legs))) or \
            be.scatter_run_bytes(node1.tensor, node2.tensor, [axes1, axes2], order) < min_run:
          order = None
      if order is not None:
        t = be.tensordot_planned(node1.tensor, node2.tensor, [axes1, axes2], result_order=order)[0]
        sources = [legs[p] for p in order]
      else:
        # (the axis order of the result is bookkeeping here: the backend may put node2's axes first)
        t, used1, used2, swapped = be.tensordot_planned(node1.tensor, node2.tensor, [axes1, axes2], order1, order2,
                                                        allow_swap=True)
        sources = [(node1, i) for i in used1] + [(node2, i) for i in used2]
        if swapped:
          sources = sources[len(used1):] + sources[:len(used1)]
    else:
      t = be.tensordot(node1.tensor, node2.tensor, [axes1, axes2])
      sources = [(node1, i) for i in range(len(node1.edges)) if i not in axes1] + \
                [(node2, i) for i in range(len(node2.edges)) if i not in axes2]
    if len(sources) == len(be.shape_tuple(t)):
      out = Node._from_contraction(t, name, be, sources)  # pylint: disable=protected-access
    else:     # (a backend that returns something else than its tensor type: the general constructor decides)
      out = Node(t, name=name, backend=be)
      _adopt_edges(out, sources)
  if output_edge_order is not None:
    output_edge_order = list(output_edge_order)
    if set(output_edge_order) != set(out.edges):
      raise ValueError(f"output edges are not equal to the remaining non-contracted edges of the "
                       f"final node. output_edge_order = {output_edge_order}, remaining = {out.edges}")
    out.reorder_edges(output_edge_order)
  if axis_names is not None:
    if len(axis_names) != len(out.edges):
      raise ValueError("axis_names does not match the rank of the result")
    out.axis_names = list(axis_names)
  return out


def contract_copy_node(copy_node: CopyNode, name: Optional[str] = None) -> Node:
  """Contract a copy node with all of its neighbours at once (network_components.py:1888-1920): the
  result has the neighbours' remaining axes, neighbour by neighbour; edges between two neighbours survive
  (as trace edges of the result)."""
  partners = copy_node.get_partners()
  out = Node(copy_node.compute_contracted_tensor(), name=name, backend=copy_node.backend)
  sources = []
  for partner in partners:
    for axis, e in enumerate(partner.edges):
      if e.node1 is copy_node or e.node2 is copy_node:
        continue
      sources.append((partner, axis))
  assert len(sources) == len(out.edges)
  _adopt_edges(out, sources)
  copy_node.edges = [Edge(copy_node, i, name=copy_node.axis_names[i]) for i in range(copy_node.rank)]
  return out


def contract_parallel(edge: Edge) -> Node:
  """Contract all edges parallel to `edge` (network_components.py:1923-1936)."""
  if edge.is_dangling():
    raise ValueError(f"Attempted to contract dangling edge: '{edge}'")
  return contract_between(edge.node1, edge.node2)


# -------------------------------------------------------------------- splitting
def _split_bookkeeping(node, left_edges, right_edges):
  if set(left_edges) | set(right_edges) != set(node.edges) or \
      len(left_edges) + len(right_edges) != len(node.edges):
    raise ValueError("left_edges and right_edges must partition the edges of the node")
  return node.tensor_from_edge_order(list(left_edges) + list(right_edges))


def split_node(node: Node, left_edges: List[Edge], right_edges: List[Edge],
               max_singular_values: Optional[int] = None, max_truncation_err: Optional[float] = None,
               relative: bool = False, left_name: Optional[str] = None, right_name: Optional[str] = None,
               edge_name: Optional[str] = None) -> Tuple[Node, Node, Any]:
  """SVD-split: node = (U sqrt(S)) -- (sqrt(S) Vh)  (network_operations.py:130-255).

  Returns (left_node, right_node, truncated_singular_values)."""
  be = node.backend
  left_sources = [(node, node.edges.index(e)) for e in left_edges]
  right_sources = [(node, node.edges.index(e)) for e in right_edges]
  t = _split_bookkeeping(node, left_edges, right_edges)
  u, s, vh, trun_vals = be.svd(t, len(left_edges), max_singular_values, max_truncation_err,
                               relative=relative)
  sqrt_s = be.sqrt(s)
  u_s = be.broadcast_right_multiplication(u, sqrt_s)
  vh_s = be.broadcast_left_multiplication(sqrt_s, vh)
  left = Node(u_s, name=left_name, backend=be)
  right = Node(vh_s, name=right_name, backend=be)
  _adopt_edges(left, left_sources + [(left, len(left_edges))])
  _adopt_edges(right, [(right, 0)] + right_sources)
  connect(left.edges[-1], right.edges[0], name=edge_name)
  node.edges = []  # the node is consumed, as in the reference (fresh_edges)
  return left, right, trun_vals


def split_node_full_svd(node: Node, left_edges: List[Edge], right_edges: List[Edge],
                        max_singular_values: Optional[int] = None,
                        max_truncation_err: Optional[float] = None, relative: bool = False,
                        left_name: Optional[str] = None, middle_name: Optional[str] = None,
                        right_name: Optional[str] = None) -> Tuple[Node, Node, Node, Any]:
  """node = U -- S -- Vh with S a diagonal matrix node (network_operations.py:446-588)."""
  be = node.backend
  left_sources = [(node, node.edges.index(e)) for e in left_edges]
  right_sources = [(node, node.edges.index(e)) for e in right_edges]
  t = _split_bookkeeping(node, left_edges, right_edges)
  u, s, vh, trun_vals = be.svd(t, len(left_edges), max_singular_values, max_truncation_err,
                               relative=relative)
  left = Node(u, name=left_name, backend=be)
  mid = Node(be.diagflat(s), name=middle_name, backend=be)
  right = Node(vh, name=right_name, backend=be)
  _adopt_edges(left, left_sources + [(left, len(left_edges))])
  _adopt_edges(right, [(right, 0)] + right_sources)
  connect(left.edges[-1], mid.edges[0])
  connect(mid.edges[1], right.edges[0])
  node.edges = []
  return left, mid, right, trun_vals


def _split_two(node, left_edges, right_edges, factor, left_name, right_name, edge_name):
  be = node.backend
  left_sources = [(node, node.edges.index(e)) for e in left_edges]
  right_sources = [(node, node.edges.index(e)) for e in right_edges]
  t = _split_bookkeeping(node, left_edges, right_edges)
  lt, rt = factor(be, t, len(left_edges))
  left = Node(lt, name=left_name, backend=be)
  right = Node(rt, name=right_name, backend=be)
  _adopt_edges(left, left_sources + [(left, len(left_edges))])
  _adopt_edges(right, [(right, 0)] + right_sources)
  connect(left.edges[-1], right.edges[0], name=edge_name)
  node.edges = []
  return left, right


def split_node_qr(node: Node, left_edges: List[Edge], right_edges: List[Edge],
                  left_name: Optional[str] = None, right_name: Optional[str] = None,
                  edge_name: Optional[str] = None) -> Tuple[Node, Node]:
  """node = Q -- R with Q orthonormal on the left edges (network_operations.py:258-349)."""
  return _split_two(node, left_edges, right_edges, lambda be, t, p: be.qr(t, p), left_name, right_name,
                    edge_name)


def split_node_rq(node: Node, left_edges: List[Edge], right_edges: List[Edge],
                  left_name: Optional[str] = None, right_name: Optional[str] = None,
                  edge_name: Optional[str] = None) -> Tuple[Node, Node]:
  """node = R -- Q with Q orthonormal on the right edges (network_operations.py:352-443)."""
  return _split_two(node, left_edges, right_edges, lambda be, t, p: be.rq(t, p), left_name, right_name,
                    edge_name)


# ------------------------------------------------------------- graph surgery
def get_parallel_edges(edge: Edge) -> Set[Edge]:
  """All edges between the two nodes of ``edge``, itself included (network_components.py:1302-1312)."""
  return get_shared_edges(edge.node1, edge.node2)


def get_all_nondangling(nodes: Iterable[Node]) -> Set[Edge]:
  return {e for n in nodes for e in n.edges if not e.is_dangling()}


def get_all_dangling(nodes: Iterable[Node]) -> List[Edge]:
  return [e for n in nodes for e in n.edges if e.is_dangling()]


def get_all_nodes(edges: Iterable[Edge]) -> Set[Node]:
  return {n for e in edges for n in e.get_nodes() if n is not None}


def get_neighbors(node: Node) -> List[Node]:
  """Nodes sharing an edge with ``node``, in axis order, without duplicates and never ``node``
  itself (network_operations.py:823-846)."""
  out: List[Node] = []
  for e in node.edges:
    if e.is_dangling() or e.is_trace():
      continue
    other = e.node2 if e.node1 is node else e.node1
    if not any(other is o for o in out):
      out.append(other)
  return out


def check_connected(nodes: Iterable[Node]) -> None:
  """ValueError("Non-connected graph") unless every node is reachable from the first
  (network_operations.py:680-694)."""
  nodes = list(nodes)
  if not set(nodes) <= reachable(nodes[0]):
    raise ValueError("Non-connected graph")


def check_correct(nodes: Iterable[Node], check_connections: bool = True) -> None:
  """Every edge slot of every node must hold an edge that points back at that (node, axis)
  (network_operations.py:641-677)."""
  nodes = list(nodes)
  for node in nodes:
    for i, edge in enumerate(node.edges):
      if edge.node1 is not node and edge.node2 is not node:
        raise ValueError("Edge '{}' does not connect to node '{}'."
                         "Edge's nodes: '{}', '{}'.".format(edge, node, edge.node1, edge.node2))
      if not ((edge.node1 is node and edge.axis1 == i) or (edge.node2 is node and edge.axis2 == i)):
        raise ValueError("Edge '{}' does not point to '{}' on the correct axis. "
                         "Edge axes: {}, {}. Node axis: {}.".format(edge, node, edge.axis1, edge.axis2, i))
  if check_connections:
    check_connected(nodes)


def disconnect(edge: Edge, edge1_name: Optional[str] = None, edge2_name: Optional[str] = None
               ) -> Tuple[Edge, Edge]:
  """Break a connected edge into two dangling ones (network_components.py:1225-1262, 2098-2113)."""
  if edge.is_dangling():
    raise ValueError("Cannot break dangling edge {}.".format(edge))
  n1, a1, n2, a2 = edge.node1, edge.axis1, edge.node2, edge.axis2
  e1 = Edge(n1, a1, name=edge1_name or '__disconnected_edge1_of_{}__'.format(edge.name))
  e2 = Edge(n2, a2, name=edge2_name or '__disconnected_edge2_of_{}__'.format(edge.name))
  n1.edges[a1] = e1
  n2.edges[a2] = e2
  return e1, e2


def remove_node(node: Node) -> Tuple[Dict[str, Edge], Dict[int, Edge]]:
  """Cut ``node`` out of its network (network_operations.py:103-127): every edge to ANOTHER node is
  broken; returns the neighbours' new dangling edges keyed by ``node``'s axis name and axis number."""
  by_name, by_axis = {}, {}
  for i, name in enumerate(node.axis_names):
    e = node.edges[i]
    if e.is_dangling() or e.is_trace():
      continue
    e1, e2 = disconnect(e)
    far = e1 if e1.node1 is not node else e2
    by_axis[i] = far
    by_name[name] = far
  return by_name, by_axis


def redirect_edge(edge: Edge, new_node: Node, old_node: Node) -> None:
  """Move the end(s) of ``edge`` that sit on ``old_node`` over to the same axis of ``new_node``;
  ``old_node`` gets a fresh dangling edge there (network_operations.py:988-1040)."""
  ends = [(n, ax) for n, ax in edge.ends() if n is old_node]
  if not ends or (edge.is_trace() and edge.node1 is not old_node):
    raise ValueError(f"edge {edge} is not pointing to old_node {old_node}")
  for _, ax in ends:
    if edge.node1 is old_node and edge.axis1 == ax:
      edge.node1 = new_node
    else:
      edge.node2 = new_node
    new_node.edges[ax] = edge
    old_node.edges[ax] = Edge(old_node, ax)


def _fold_trailing(node: Node, back_axes: Sequence[int], back_shape: Sequence[int]) -> int:
  """Permute ``back_axes`` (in this order) behind the other axes of ``node`` and reshape that
  trailing block to ``back_shape``, in place.  The untouched leading axes keep edges and names;
  every trailing axis gets a fresh dangling edge.  Returns the number of leading axes."""
  be = node.backend
  front = [i for i in range(len(node.edges)) if i not in back_axes]
  node.reorder_axes(front + list(back_axes))
  lead = tuple(node.shape[:len(front)])
  node.tensor = be.reshape(node.tensor, lead + tuple(int(d) for d in back_shape))
  node.edges = node.edges[:len(front)]
  node.axis_names = node.axis_names[:len(front)]
  for k in range(len(back_shape)):
    node.edges.append(Edge(node, len(front) + k))
    node.axis_names.append(str(len(front) + k))
  return len(front)


def _same_backend(nodes):
  names = {n.backend.name for n in nodes if n is not None}
  if len(names) > 1:
    raise ValueError("Not all backends are the same.")


def flatten_edges(edges: List[Edge], new_edge_name: Optional[str] = None) -> Edge:
  """Merge several edges that join the same node(s) into one edge whose dimension is the product
  (network_components.py:1367-1456; trace edges 1325-1364).  The node tensors are permuted
  (merged axes last, in the order given) and reshaped in place."""
  edges = list(edges)
  if not edges:
    raise ValueError("At least 1 edge must be given.")
  _same_backend([n for e in edges for n in e.get_nodes()])
  if len(edges) == 1:
    return edges[0]
  first = {id(n) for n in edges[0].get_nodes()}
  for e in edges:
    if {id(n) for n in e.get_nodes()} != first:
      raise ValueError("Two edges do not share the same nodes. '{}'s nodes: '{}', '{}'. '{}'s nodes: '{}', '{}'"
                       .format(edges[0], edges[0].node1, edges[0].node2, e, e.node1, e.node2))
  dim = math.prod(int(e.dimension) for e in edges)
  if edges[0].is_trace():
    node = edges[0].node1
    back = [min(e.axis1, e.axis2) for e in edges] + [max(e.axis1, e.axis2) for e in edges]
    k = _fold_trailing(node, back, (dim, dim))
    return connect(node.edges[k], node.edges[k + 1], new_edge_name)
  fresh = []
  for node in (edges[0].node1, edges[0].node2):
    if node is None:
      continue
    back = [e.axis1 if e.node1 is node else e.axis2 for e in edges]
    k = _fold_trailing(node, back, (dim,))
    node.edges[k].name = new_edge_name if new_edge_name is not None else node.edges[k].name
    fresh.append(node.edges[k])
  if len(fresh) == 1:
    return fresh[0]
  return connect(fresh[0], fresh[1], new_edge_name)


def flatten_edges_between(node1: Node, node2: Node) -> Optional[Edge]:
  """One edge in place of all edges between two nodes; None if they share none
  (network_components.py:1459-1477)."""
  shared = get_shared_edges(node1, node2)
  if not shared:
    return None
  owner = node1
  return flatten_edges(sorted(shared, key=lambda e: e.axis1 if e.node1 is owner else e.axis2))


def flatten_all_edges(nodes: Iterable[Node]) -> List[Edge]:
  """Flatten every group of parallel (or parallel trace) edges in the network; returns one edge per
  connected pair (network_components.py:1480-1492)."""
  nodes = list(nodes)
  out, done = [], set()
  for node in nodes:
    for e in list(node.edges):
      if e.is_dangling():
        continue
      pair = frozenset((id(e.node1), id(e.node2)))
      if pair in done:
        continue
      done.add(pair)
      out.append(flatten_edges_between(e.node1, e.node2))
  return out


def split_edge(edge: Edge, shape: Tuple[int, ...], new_edge_names: Optional[List[str]] = None) -> List[Edge]:
  """Inverse of flattening: replace ``edge`` by ``len(shape)`` edges of the given dimensions
  (network_components.py:1495-1633).  Works for connected, dangling and trace edges."""
  shape = tuple(int(d) for d in shape)
  if math.prod(shape) != edge.dimension:
    raise ValueError("Edge {} with dimension {} cannot be split according to shape {}."
                     .format(edge, edge.dimension, shape))
  if len(shape) == 1:
    return [edge]
  name = lambda i: new_edge_names[i] if new_edge_names is not None else None
  if edge.is_trace():
    node = edge.node1
    k = _fold_trailing(node, [min(edge.axis1, edge.axis2), max(edge.axis1, edge.axis2)], shape + shape)
    return [connect(node.edges[k + i], node.edges[k + len(shape) + i], name(i)) for i in range(len(shape))]
  _same_backend(edge.get_nodes())
  halves = []
  for node in (edge.node1, edge.node2):
    if node is None:
      continue
    k = _fold_trailing(node, [edge.axis1 if edge.node1 is node else edge.axis2], shape)
    for i in range(len(shape)):
      if name(i) is not None:
        node.edges[k + i].name = name(i)
        node.axis_names[k + i] = name(i)
    halves.append(node.edges[k:])
  if len(halves) == 1:
    return list(halves[0])
  return [connect(halves[0][i], halves[1][i], name(i)) for i in range(len(shape))]


def replicate_nodes(nodes: Iterable[Node], conjugate: bool = False) -> List[Node]:
  """Copies of ``nodes`` wired like the originals (network_operations.py:86-100)."""
  nodes = list(nodes)
  node_map, _ = copy(nodes, conjugate=conjugate)
  return [node_map[n] for n in nodes]


def reduced_density(traced_out_edges: Iterable[Edge]) -> Tuple[Dict[Node, Node], Dict[Edge, Edge]]:
  """Turn a pure-state network into its reduced density matrix (network_operations.py:753-791): the
  whole reachable network is copied conjugated and each edge in ``traced_out_edges`` is joined to
  its copy.  Returns (node -> conjugate copy, edge -> copy) with the traced edges mapped to the new
  connecting edges."""
  traced = list(traced_out_edges)
  if any(not e.is_dangling() for e in traced):
    raise ValueError("traced_out_edges must only include dangling edges!")
  seen: Dict[int, Node] = {}
  for start in get_all_nodes(traced):
    for n in reachable(start):
      seen[id(n)] = n
  node_map, edge_map = copy(seen.values(), conjugate=True)
  for e in traced:
    edge_map[e] = connect(edge_map[e], e)
  return node_map, edge_map


def from_topology(topology: str, tensors: Sequence[Any], backend=None) -> List[Node]:
  """Nodes wired as the left side of an einsum expression says, e.g. ``"xy,yz,zx"`` (utils.py:115-158):
  one letter per axis, equal letters are connected, axis names are the letters."""
  parts = topology.split(",")
  if len(parts) != len(tensors):
    raise ValueError("topology and number of tensors is mismatched")
  open_edges: Dict[str, Edge] = {}
  nodes = []
  for letters, tensor in zip(parts, tensors):
    if len(letters) != len(tensor.shape):
      raise ValueError(f"{letters} does not match shape {tensor.shape}")
    node = Node(tensor, axis_names=list(letters), backend=backend)
    for c in letters:
      open_edges[c] = connect(open_edges[c], node[c]) if c in open_edges else node[c]
    nodes.append(node)
  return nodes


def switch_backend(nodes: Iterable[Node], new_backend) -> None:
  """Move the tensors of ``nodes`` to ``new_backend`` (network_operations.py:794-820): host copy out
  of the old backend (``__array__``), ingest by the new one."""
  be = _resolve_backend(new_backend)
  for node in nodes:
    if node.backend is be:
      continue
    node.tensor = be.convert_to_tensor(np.asarray(node.tensor))
    node.backend = be


# ------------------------------------------------------------------ copy / slice
def copy(nodes: Iterable[Node], conjugate: bool = False) -> Tuple[Dict[Node, Node], Dict[Edge, Edge]]:
  """Structure-preserving copy of a sub-network (network_operations.py:32-83).

  Tensors are shared, not duplicated (they are immutable on the backend)."""
  nodes = list(nodes)
  node_map: Dict[Node, Node] = {}
  for n in nodes:
    t = n.backend.conj(n.tensor) if conjugate else n.tensor
    node_map[n] = Node(t, name=n.name, axis_names=list(n.axis_names), backend=n.backend)
  edge_map: Dict[Edge, Edge] = {}
  for e in get_all_edges(nodes):
    ends = [(nd, ax) for nd, ax in e.ends() if nd in node_map]
    if len(ends) == 2:
      new = connect(node_map[ends[0][0]].edges[ends[0][1]], node_map[ends[1][0]].edges[ends[1][1]],
                    name=e.name)
    else:
      new = node_map[ends[0][0]].edges[ends[0][1]]
      new.name = e.name
    edge_map[e] = new
  return node_map, edge_map


def slice_edge(edge: Edge, start_index: int, length: int) -> Edge:
  """Restrict `edge` to indices [start, start+length) in place
  (network_components.py:1636-1682)."""
  if start_index < 0 or length <= 0 or start_index + length > edge.dimension:
    raise ValueError(f"slice [{start_index}, {start_index + length}) is out of range for "
                     f"edge of dimension {edge.dimension}")
  for node, axis in edge.ends():
    shape = node.shape
    starts = [0] * len(shape)
    sizes = list(shape)
    starts[axis] = start_index
    sizes[axis] = length
    node.tensor = node.backend.slice(node.tensor, tuple(starts), tuple(sizes))
  return edge


# ------------------------------------------------------------------ wire format (JSON)
def nodes_to_json(nodes: Sequence[Node], edge_binding: Optional[Dict[str, Any]] = None) -> str:
  """JSON string of a network: same schema as the reference's ``nodes_to_json``
  (network_operations.py:880-941) -- nodes with name / axis_names / backend / serialised tensor
  (``backend.serialize_tensor``: np.save bytes as a latin-1 string), edges with their two
  (node id, axis) ends (``None`` for a dangling end or an end outside ``nodes``) and optional
  named edge bindings -- so files travel between the two libraries."""
  import json  # pylint: disable=import-outside-toplevel
  nodes = list(nodes)
  node_id = {id(n): i for i, n in enumerate(nodes)}
  out = {"nodes": [], "edges": []}
  for i, n in enumerate(nodes):
    out["nodes"].append({"id": i, "attributes": {"name": n.name, "axis_names": list(n.axis_names),
                                                 "backend": n.backend.name,
                                                 "tensor": n.backend.serialize_tensor(n.tensor)}})
  edges, seen = [], set()
  for n in nodes:                     # deterministic order: by first appearance
    for e in n.edges:
      if id(e) not in seen:
        seen.add(id(e))
        edges.append(e)
  edge_id = {id(e): i for i, e in enumerate(edges)}
  for i, e in enumerate(edges):
    ids = [node_id.get(id(e.node1)), node_id.get(id(e.node2)) if e.node2 is not None else None]
    axes = [e.axis1 if ids[0] is not None else None, e.axis2 if ids[1] is not None else None]
    out["edges"].append({"id": i, "node_ids": ids, "attributes": {"name": e.name, "axes": axes}})
  if edge_binding:
    binding = {}
    for k, v in edge_binding.items():
      if not isinstance(k, str):
        raise TypeError("Edge binding dict must have string keys")
      v = [v] if isinstance(v, Edge) else list(v)
      if not all(isinstance(x, Edge) for x in v):
        raise TypeError("Edge binding dict must have values of type Edge or Iterable[Edge]")
      kept = [edge_id[id(x)] for x in v if id(x) in edge_id]
      if kept:
        binding[k] = kept
    if binding:
      out["edge_binding"] = binding
  return json.dumps(out)


def nodes_from_json(json_str: str, backend=None) -> Tuple[List[Node], Dict[str, Tuple[Edge, ...]]]:
  """Rebuild a network from ``nodes_to_json`` output of this library OR of the reference
  (network_operations.py:944-985).  Tensors are deserialised by ``backend`` when given (e.g. a
  file written by the NumPy backend loaded straight into HBM), else by the backend named in the
  file."""
  import json  # pylint: disable=import-outside-toplevel
  data = json.loads(json_str)
  nodes, by_id = [], {}
  for rec in data["nodes"]:
    attr = rec["attributes"]
    be = _resolve_backend(backend if backend is not None else attr["backend"])
    node = Node(be.deserialize_tensor(attr["tensor"]), name=attr.get("name"), axis_names=attr.get("axis_names"),
                backend=be)
    nodes.append(node)
    by_id[rec["id"]] = node
  lookup = {}
  for rec in data["edges"]:
    ends = [(by_id.get(nid), ax) for nid, ax in zip(rec["node_ids"], rec["attributes"]["axes"])]
    ends = [(n, ax) for n, ax in ends if n is not None and ax is not None]
    name = rec["attributes"].get("name")
    if len(ends) == 2:
      (n1, a1), (n2, a2) = ends
      edge = Edge(n1, a1, name=name, node2=n2, axis2=a2)
      n1.edges[a1] = edge
      n2.edges[a2] = edge
    else:
      (n1, a1), = ends
      edge = Edge(n1, a1, name=name)
      n1.edges[a1] = edge
    lookup[rec["id"]] = edge
  binding = {k: tuple(lookup[i] for i in v) for k, v in data.get("edge_binding", {}).items()}
  return nodes, binding
