"""Sequential numpy restatement of the PVector COO constructor loop
(Interfaces.jl:1899-1907) and of the reads and writes of local_view /
global_view (1994-2069), in the element type: the expected values of
tests/test_gpu_vec_coo.py.  Every operation is one scalar add or store per
entry, in input order."""
import numpy as np


def scatter_add(values, lids, V):
    """values[lid] += V[i] for i in input order (1902-1905); lids 1-based.
    Returns values (modified in place)."""
    V = np.asarray(V, dtype=values.dtype)
    for i, lid in enumerate(np.asarray(lids, dtype=np.int64)):
        values[lid - 1] = values[lid - 1] + V[i]
    return values


def from_coo(nlids, lids, V, dtype):
    """fill!(values, zero(T)) then the loop (1900-1906)"""
    return scatter_add(np.zeros(nlids, dtype=dtype), lids, V)


def scatter_set(values, lids, V):
    """values[lid] = V[i] in input order: the last entry of a lid stays"""
    V = np.asarray(V, dtype=values.dtype)
    for i, lid in enumerate(np.asarray(lids, dtype=np.int64)):
        values[lid - 1] = V[i]
    return values


def gather(values, lids):
    """values[lid], or zero(T) where lid < 1 (the LocalView read, 2019-2026)"""
    lids = np.asarray(lids, dtype=np.int64)
    out = np.zeros(len(lids), dtype=values.dtype)
    ok = lids > 0
    out[ok] = values[lids[ok] - 1]
    return out


def to_lids(lid_to_gid, gids):
    """gid_to_lid[gid] (1-based), 0 where the gid is not a local id"""
    table = {int(g): l + 1 for l, g in enumerate(lid_to_gid)}
    return np.array([table.get(int(g), 0) for g in gids], dtype=np.int64)


def bits(a):
    """the values as unsigned integers: equality of these is bit identity
    (sign of zero and NaN payloads included)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.real.dtype.itemsize == 4 else np.uint64)
