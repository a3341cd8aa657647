"""Loop subdivision surfaces (include/fountain_hip_subdiv.h): a triangle control mesh refined `levels` times on the GPU, its vertices moved
to their limit positions and given limit normals -- `Shape "loopsubdiv"` of the PBRT reader and SceneBuilder.shape("loopsubdiv", ...).

  info(be, idx, n_vertices, levels)               -> A.ftn_subdiv_info: the counts of every level (validates the topology; no GPU)
  loop_subdivide(be, P, idx, levels, device=-1)   -> (P [V, 3] float32 limit positions, N [V, 3] float32 normals, idx [F, 3] uint32)
  loop_subdivide_cpu(be, P, idx, levels)          -> the same from the host twin, bit-identical to the GPU

P is [n, 3] float32 and idx [m, 3] uint32, in the space of the input.  The reference's loop_subdiv.rs ends in unimplemented!(), so the CPU
oracle has no twin of these calls: given the oracle backend they run the product library's host twin (info and loop_subdivide_cpu) --
loop_subdivide itself needs the product backend.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._nontwin import bind, ptr as _ptr
from .api import default_backend


def _lib(be):
    be = default_backend() if be is None or be.is_oracle else be
    return be, bind(be, A.EXTENSIONS["subdiv"])


def _cage(P, idx):
    P = np.ascontiguousarray(P, dtype=np.float32)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    if P.ndim != 2 or P.shape[1] != 3 or idx.ndim != 2 or idx.shape[1] != 3:
        raise ValueError("expected P [n, 3] and indices [m, 3], got %r and %r" % (P.shape, idx.shape))
    return P, idx


def info(be, idx, n_vertices, levels):
    """ftn_loop_subdivide_info: validates the control mesh and returns the counts of every level."""
    be, lib = _lib(be)
    idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1, 3)
    out = A.ftn_subdiv_info()
    be.check(lib.ftn_loop_subdivide_info(_ptr(idx), int(n_vertices), idx.shape[0], int(levels), C.byref(out)))
    return out


def _run(be, P, idx, levels, device):
    P, idx = _cage(P, idx)
    i = info(be, idx, P.shape[0], levels)
    be, lib = _lib(be)
    nv, nf = i.n_vertices[levels], i.n_faces[levels]
    out_P, out_N, out_idx = np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32), np.empty((nf, 3), np.uint32)
    args = (_ptr(P), P.shape[0], _ptr(idx), idx.shape[0], int(levels), _ptr(out_P), _ptr(out_N), _ptr(out_idx))
    be.check(lib.ftn_loop_subdivide_cpu(*args) if device is None else lib.ftn_loop_subdivide(*(args + (device,))))
    return out_P, out_N, out_idx


def loop_subdivide(be, P, idx, levels, device=-1):
    """ftn_loop_subdivide: the refined mesh's limit positions, normals and indices, computed on GPU `device`."""
    if be is not None and be.is_oracle:
        from .api import FountainError
        raise FountainError(A.FTN_ERR_UNSUPPORTED, "loop_subdivide runs on the GPU of the product library: the oracle has no twin (use loop_subdivide_cpu)")
    return _run(be, P, idx, levels, device)


def loop_subdivide_cpu(be, P, idx, levels):
    """ftn_loop_subdivide_cpu: the host twin (the same bits)."""
    return _run(be, P, idx, levels, None)
