"""ctypes binding of the native tiled driver (include/vgs_tiles.h = csrc/tiles.cpp, libvgs_tiles.so): one process per GPU, spatial
tiles, ONE all-gather of boundary records per run.  This is the product's multi-GPU path; `dist.py` is its Python
twin and stays as the test harness.

Communicators (the library's three kinds):
  * `rccl_comm(...)`            an ncclComm_t this process creates itself through librccl (ncclGetUniqueId on rank 0, the 128 id bytes
                                handed to the other ranks by the caller -- bench.py uses torch.distributed's store for that);
  * `NativeTiles.with_callbacks` the caller's own host transport (e.g. torch.distributed over gloo: two processes on ONE GPU, which
                                RCCL refuses);
  * `LocalGroup`                threads of one process (tests).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import VgsError, VgsParams

_HERE = os.path.dirname(os.path.abspath(__file__))
_TL = None
_RCCL = None

T_NAMES = ("grid", "stages", "records", "exchange", "merge", "labels", "total")
D_NAMES = ("moments", "exchange", "fold", "algebra", "total")   # vgs_tiles_get_descriptor_times
G_NAMES = ("halo", "own", "exchange", "fold", "total")          # vgs_tiles_get_graph_times
B_NAMES = ("extents", "exchange", "fold", "finish", "total")    # vgs_tiles_get_box_times
F_NAMES = ("own", "exchange", "fold", "finish", "total")        # vgs_tiles_get_field_times
C_NAMES = ("own", "exchange", "tables", "total")                # vgs_tiles_get_compare_times
R_NAMES = ("band", "exchange", "table", "refine", "total")      # vgs_tiles_get_refine_times
L_NAMES = ("own", "exchange", "fold", "finish", "total")        # vgs_tiles_get_point_label_times
LG_NAMES = ("own", "exchange1", "table", "exchange2", "fold", "total")   # vgs_tiles_get_label_graph_times
CC_NAMES = ("own", "exchange1", "link", "exchange2", "fold", "apply", "total")   # vgs_tiles_get_point_label_component_times
# (field, dtype, table) of vgs_tiles_get_point_label_components, in its argument order: Engine.COMPONENT_FIELDS with the shared-grid code
# of a part's first node in place of the node id
COMPONENT_FIELDS = (("part_of_point", np.int32, "points"), ("part_label", np.int32, "parts"), ("part_points", np.int64, "parts"),
                    ("part_nodes", np.int32, "parts"), ("part_first_code", np.uint64, "parts"), ("label_first", np.int64, "first"),
                    ("label_largest", np.int32, "labels"))
# vgs_tiles_refine_point_labels' counts, all the rank's share
REFINE_COUNTS = ("working_nodes", "points_examined", "points_changed", "points_filled", "points_beyond_strip")
# per (record / row, channel): (field, dtype) of vgs_get_own_segment_field_moments and vgs_tiles_fold_field_moments, in their argument order
FIELD_MOMENT_FIELDS = (("n_valid", np.int64), ("anchor", np.float64), ("s1", np.float64), ("s2", np.float64), ("vmin", np.float32), ("vmax", np.float32))
# per record / row: (field, dtype, values) of vgs_get_own_segment_moments and vgs_tiles_fold_moments, in their argument order
MOMENT_FIELDS = (("n_points", np.int64, 1), ("n_nodes", np.int32, 1), ("bbox6", np.float32, 6), ("anchor3", np.float32, 3), ("s9", np.float64, 9))
COMM_RCCL, COMM_LOCAL, COMM_CALLBACKS = 0, 1, 2
OPT_STRICT_REGION = 1

_AG_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
_BC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int)


class _Callbacks(C.Structure):
    _fields_ = [("user", C.c_void_p), ("all_gather", _AG_FN), ("bcast", _BC_FN)]


def lib():
    """libvgs_tiles.so (loads libvgs_hip.so first: it links against it).  No GPU is needed to load it."""
    global _TL
    if _TL is None:
        _lib.lib()
        L = C.CDLL(os.path.join(_HERE, "libvgs_tiles.so"))
        P = C.c_void_p
        L.vgs_tiles_create.restype = C.c_int
        L.vgs_tiles_create.argtypes = [P, C.c_int, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, P]
        L.vgs_tiles_destroy.restype = None
        L.vgs_tiles_destroy.argtypes = [P]
        L.vgs_tiles_last_error_string.restype = C.c_char_p
        L.vgs_tiles_last_error_string.argtypes = [P]
        L.vgs_tiles_context.restype = P
        L.vgs_tiles_context.argtypes = [P]
        L.vgs_tiles_set_option.restype = C.c_int
        L.vgs_tiles_set_option.argtypes = [P, C.c_int32, C.c_int64]
        L.vgs_tiles_set_points.restype = C.c_int
        L.vgs_tiles_set_points.argtypes = [P, P, C.c_int64, C.c_int32]
        L.vgs_tiles_run.restype = C.c_int
        L.vgs_tiles_run.argtypes = [P]
        L.vgs_tiles_get_times.restype = C.c_int
        L.vgs_tiles_get_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_get_point_labels.restype = C.c_int
        L.vgs_tiles_get_point_labels.argtypes = [P, P, P]
        L.vgs_tiles_get_info.restype = C.c_int
        L.vgs_tiles_get_info.argtypes = [P, P, P, P]
        L.vgs_tiles_get_exchange.restype = C.c_int
        L.vgs_tiles_get_exchange.argtypes = [P, P, P, P]
        L.vgs_tiles_local_group_create.restype = C.c_int
        L.vgs_tiles_local_group_create.argtypes = [C.c_int, P]
        L.vgs_tiles_local_group_destroy.restype = None
        L.vgs_tiles_local_group_destroy.argtypes = [P]
        L.vgs_tiles_local_group_abort.restype = None
        L.vgs_tiles_local_group_abort.argtypes = [P]
        L.vgs_tiles_merge_boundary.restype = C.c_int
        L.vgs_tiles_merge_boundary.argtypes = [C.c_int, P, P, P, P, P, C.c_int, P, P, P, P, P]
        L.vgs_tiles_get_segment_descriptors.restype = C.c_int
        L.vgs_tiles_get_segment_descriptors.argtypes = [P, P, P, P, P, P, P, P, P, P]
        L.vgs_tiles_get_descriptor_times.restype = C.c_int
        L.vgs_tiles_get_descriptor_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_fold_moments.restype = C.c_int
        L.vgs_tiles_fold_moments.argtypes = [C.c_int, P, P, P, P, P, P, P, C.c_int64, P, P, P, P, P]
        L.vgs_tiles_get_segment_graph.restype = C.c_int
        L.vgs_tiles_get_segment_graph.argtypes = [P, P, P, P, P, P, P, P, P]
        L.vgs_tiles_get_graph_times.restype = C.c_int
        L.vgs_tiles_get_graph_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_get_graph_payload.restype = C.c_int
        L.vgs_tiles_get_graph_payload.argtypes = [P, P, P, P]
        L.vgs_tiles_fold_edges.restype = C.c_int
        L.vgs_tiles_fold_edges.argtypes = [C.c_int, P, P, P, P, P, P, P, P, C.c_int64, P, P, P, P, P, P, P, P]
        L.vgs_tiles_get_segment_boxes.restype = C.c_int
        L.vgs_tiles_get_segment_boxes.argtypes = [P, C.c_int32, P, P, P, P, P, P]
        L.vgs_tiles_get_box_times.restype = C.c_int
        L.vgs_tiles_get_box_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_fold_extents.restype = C.c_int
        L.vgs_tiles_fold_extents.argtypes = [C.c_int, P, P, P, P, C.c_int64, P, P, P]
        for name in ("vgs_tiles_segment_field_stats", "vgs_tiles_segment_field_stats_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, C.c_int32, C.c_int64, P, P, P, P, P, P, P]
        for name in ("vgs_tiles_segment_class_histogram", "vgs_tiles_segment_class_histogram_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, C.c_int32, P, P, P, P, P]
        L.vgs_tiles_get_field_times.restype = C.c_int
        L.vgs_tiles_get_field_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_get_field_payload.restype = C.c_int
        L.vgs_tiles_get_field_payload.argtypes = [P, P, P]
        for name in ("vgs_tiles_compare_labels", "vgs_tiles_compare_labels_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, P, P, P, P]
        L.vgs_tiles_get_label_comparison.restype = C.c_int
        L.vgs_tiles_get_label_comparison.argtypes = [P] + [P] * 14
        L.vgs_tiles_get_compare_times.restype = C.c_int
        L.vgs_tiles_get_compare_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_get_compare_payload.restype = C.c_int
        L.vgs_tiles_get_compare_payload.argtypes = [P, P, P]
        L.vgs_tiles_refine_point_labels.restype = C.c_int
        L.vgs_tiles_refine_point_labels.argtypes = [P, C.POINTER(_lib.VgsRefineParams), P]
        L.vgs_tiles_get_refined_labels.restype = C.c_int
        L.vgs_tiles_get_refined_labels.argtypes = [P, P]
        L.vgs_tiles_get_refine_times.restype = C.c_int
        L.vgs_tiles_get_refine_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_get_refine_payload.restype = C.c_int
        L.vgs_tiles_get_refine_payload.argtypes = [P, P, P]
        for name in ("vgs_tiles_point_label_descriptors", "vgs_tiles_point_label_descriptors_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, C.c_int64] + [P] * 9
        for name in ("vgs_tiles_point_label_boxes", "vgs_tiles_point_label_boxes_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, C.c_int64, C.c_int32, P, P, P, P, P]
        for name in ("vgs_tiles_compare_point_labels", "vgs_tiles_compare_point_labels_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, P, C.c_int64, P, P, P]
        for name in ("vgs_tiles_point_label_field_stats", "vgs_tiles_point_label_field_stats_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, P, C.c_int64, C.c_int32, C.c_int64] + [P] * 7
        for name in ("vgs_tiles_point_label_class_histogram", "vgs_tiles_point_label_class_histogram_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, P, C.c_int64, C.c_int32] + [P] * 5
        L.vgs_tiles_fold_label_pairs.restype = C.c_int
        L.vgs_tiles_fold_label_pairs.argtypes = [C.c_int, P, P, P, C.c_int64, P]
        L.vgs_tiles_get_point_label_times.restype = C.c_int
        L.vgs_tiles_get_point_label_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_get_point_label_payload.restype = C.c_int
        L.vgs_tiles_get_point_label_payload.argtypes = [P, P, P, P]
        for name in ("vgs_tiles_point_label_components", "vgs_tiles_point_label_components_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, C.c_int64, P, P]
        L.vgs_tiles_get_point_label_components.restype = C.c_int
        L.vgs_tiles_get_point_label_components.argtypes = [P] * 8
        L.vgs_tiles_fold_label_parts.restype = C.c_int
        L.vgs_tiles_fold_label_parts.argtypes = [C.c_int, C.c_int64] + [P] * 21
        L.vgs_tiles_get_point_label_component_times.restype = C.c_int
        L.vgs_tiles_get_point_label_component_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_get_point_label_component_payload.restype = C.c_int
        L.vgs_tiles_get_point_label_component_payload.argtypes = [P, P, P, P, P]
        for name in ("vgs_tiles_point_label_graph", "vgs_tiles_point_label_graph_device"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [P, P, C.c_int64, C.c_int64, P, P]
        L.vgs_tiles_get_point_label_graph.restype = C.c_int
        L.vgs_tiles_get_point_label_graph.argtypes = [P] * 9
        L.vgs_tiles_fold_label_edges.restype = C.c_int
        L.vgs_tiles_fold_label_edges.argtypes = [C.c_int, C.c_int64] + [P] * 18
        L.vgs_tiles_get_label_graph_times.restype = C.c_int
        L.vgs_tiles_get_label_graph_times.argtypes = [P, P, C.c_int32]
        L.vgs_tiles_get_label_graph_payload.restype = C.c_int
        L.vgs_tiles_get_label_graph_payload.argtypes = [P, P, P, P, P]
        L.vgs_tiles_fold_field_moments.restype = C.c_int
        L.vgs_tiles_fold_field_moments.argtypes = [C.c_int, P, P, C.c_int32, P, P, P, P, P, P, C.c_int64, P, P, P, P, P, P]
        L.vgs_tiles_fold_class_counts.restype = C.c_int
        L.vgs_tiles_fold_class_counts.argtypes = [C.c_int, P, P, C.c_int32, P, P, C.c_int64, P, P, P, P]
        _TL = L
    return _TL


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def fold_moments(records, K):
    """vgs_tiles_fold_moments (host arithmetic, no GPU): records[r] = rank r's dict of MOMENT_FIELDS arrays plus "label" (int32), as
    vgs_get_own_segment_moments gives them; returns the K folded rows as a dict of MOMENT_FIELDS arrays."""
    world = len(records)
    n = [len(r["label"]) for r in records]
    off = np.zeros(world + 1, dtype=np.int64)
    off[1:] = np.cumsum(n)
    flat = {"label": np.ascontiguousarray(np.concatenate([r["label"] for r in records]).astype(np.int32))}
    for name, dt, w in MOMENT_FIELDS:
        flat[name] = np.ascontiguousarray(np.concatenate([np.asarray(r[name], dtype=dt).reshape(-1, w) for r in records]).reshape(-1))
    out = {name: np.zeros((K, w) if w > 1 else K, dtype=dt) for name, dt, w in MOMENT_FIELDS}
    st = lib().vgs_tiles_fold_moments(world, _vp(off), _vp(flat["label"]), *(_vp(flat[name]) for name, _, _ in MOMENT_FIELDS), int(K),
                                      *(_vp(out[name]) for name, _, _ in MOMENT_FIELDS))
    if st != 0:
        raise VgsError(st, "vgs_tiles_fold_moments")
    return out


def _graph_fields():
    from .api import Engine
    return Engine.GRAPH_FIELDS


def fold_edges(tables, K):
    """vgs_tiles_fold_edges (host arithmetic, no GPU): tables[r] = rank r's partial edge table, a dict of Engine.GRAPH_FIELDS arrays
    ascending in (a, b); returns the folded table over the labels 0 .. K-1 as the same dict."""
    F = _graph_fields()
    world = len(tables)
    n = [np.asarray(t["seg_ab"]).reshape(-1, 2).shape[0] for t in tables]
    off = np.zeros(world + 1, dtype=np.int64)
    off[1:] = np.cumsum(n)
    flat = {name: np.ascontiguousarray(np.concatenate([np.asarray(t[name], dtype=dt).reshape(-1, w) for t in tables]).reshape(-1))
            for name, dt, w in F}
    total = max(int(off[-1]), 1)
    out = {name: np.zeros((total, w) if w > 1 else total, dtype=dt) for name, dt, w in F}
    E = C.c_int64(0)
    st = lib().vgs_tiles_fold_edges(world, _vp(off), *(_vp(flat[name]) for name, _, _ in F), int(K), C.byref(E),
                                    *(_vp(out[name]) for name, _, _ in F))
    if st != 0:
        raise VgsError(st, "vgs_tiles_fold_edges")
    return {name: a[:E.value].copy() for name, a in out.items()}


def fold_extents(records, K):
    """vgs_tiles_fold_extents (host arithmetic, no GPU): records[r] = rank r's dict of label (int32), lo3 and hi3 (float64, 3 per
    record), as vgs_get_own_segment_extents gives them; returns the K folded rows as a dict of lo3 (K, 3), hi3 (K, 3) and reached (K,
    uint8: a record names the label)."""
    world = len(records)
    n = [len(r["label"]) for r in records]
    off = np.zeros(world + 1, dtype=np.int64)
    off[1:] = np.cumsum(n)
    lab = np.ascontiguousarray(np.concatenate([np.asarray(r["label"]) for r in records]).astype(np.int32))
    lo = np.ascontiguousarray(np.concatenate([np.asarray(r["lo3"], dtype=np.float64).reshape(-1, 3) for r in records]).reshape(-1))
    hi = np.ascontiguousarray(np.concatenate([np.asarray(r["hi3"], dtype=np.float64).reshape(-1, 3) for r in records]).reshape(-1))
    K = int(K)
    out = {"lo3": np.zeros((max(K, 1), 3)), "hi3": np.zeros((max(K, 1), 3)), "reached": np.zeros(max(K, 1), dtype=np.uint8)}
    st = lib().vgs_tiles_fold_extents(world, _vp(off), _vp(lab), _vp(lo), _vp(hi), K, _vp(out["lo3"]), _vp(out["hi3"]), _vp(out["reached"]))
    if st != 0:
        raise VgsError(st, "vgs_tiles_fold_extents")
    return {name: a[:max(K, 0)] for name, a in out.items()}


def fold_label_pairs(records, K):
    """vgs_tiles_fold_label_pairs (host arithmetic, no GPU): records[r] = rank r's dict of pair_code (uint64) and pair_label (int32), as
    vgs_get_own_point_label_moments gives them; returns n_nodes_add (K,) int32: per label the distinct (code, label) pairs of all ranks."""
    world = len(records)
    K = int(K)
    off = np.zeros(world + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r["pair_label"]) for r in records])
    code = np.ascontiguousarray(np.concatenate([np.asarray(r["pair_code"], dtype=np.uint64).reshape(-1) for r in records]))
    lab = np.ascontiguousarray(np.concatenate([np.asarray(r["pair_label"], dtype=np.int32).reshape(-1) for r in records]))
    out = np.zeros(max(K, 1), dtype=np.int32)
    st = lib().vgs_tiles_fold_label_pairs(world, _vp(off), _vp(code), _vp(lab), K, _vp(out))
    if st != 0:
        raise VgsError(st, "vgs_tiles_fold_label_pairs")
    return out[:max(K, 0)]


def fold_label_parts(records, K):
    """vgs_tiles_fold_label_parts (host arithmetic, no GPU): step 5 of vgs_tiles_point_label_components.  records[r] = rank r's dict of
    part_label (int32), part_points (int64), part_nodes (int32), part_first_code (uint64), band_code (uint64), band_label, band_part
    (int32) -- what NativeTiles.own_point_label_parts() gives -- and link_own, link_rank, link_part (int32; absent = no link).  Returns
    the global table as a dict: part_label, part_points, part_nodes, part_first_code, label_first (K + 1), label_largest (K), n_parts,
    and map, the list of every rank's array from local to global part."""
    world, K = len(records), int(K)

    def cat(name, dt):
        return np.ascontiguousarray(np.concatenate([np.asarray(r.get(name, ()), dtype=dt).reshape(-1) for r in records] + [np.zeros(0, dtype=dt)]))

    def off(name):
        o = np.zeros(world + 1, dtype=np.int64)
        o[1:] = np.cumsum([len(r.get(name, ())) for r in records])
        return o
    p_off, b_off, l_off = off("part_label"), off("band_label"), off("link_own")
    ins = [cat("part_label", np.int32), cat("part_points", np.int64), cat("part_nodes", np.int32), cat("part_first_code", np.uint64)]
    band = [cat("band_code", np.uint64), cat("band_label", np.int32), cat("band_part", np.int32)]
    link = [cat("link_own", np.int32), cat("link_rank", np.int32), cat("link_part", np.int32)]
    P, k = max(int(p_off[-1]), 1), max(K, 0)
    n_parts = C.c_int64(0)
    out = {"map": np.zeros(P, dtype=np.int32), "part_label": np.zeros(P, dtype=np.int32), "part_points": np.zeros(P, dtype=np.int64),
           "part_nodes": np.zeros(P, dtype=np.int32), "part_first_code": np.zeros(P, dtype=np.uint64),
           "label_first": np.zeros(k + 1, dtype=np.int64), "label_largest": np.zeros(max(k, 1), dtype=np.int32)}
    st = lib().vgs_tiles_fold_label_parts(world, K, _vp(p_off), *(_vp(a) for a in ins), _vp(b_off), *(_vp(a) for a in band), _vp(l_off),
                                          *(_vp(a) for a in link), C.byref(n_parts), *(_vp(out[name]) for name in out))
    if st != 0:
        raise VgsError(st, "vgs_tiles_fold_label_parts")
    c = int(n_parts.value)
    res = {name: out[name][:c] for name in ("part_label", "part_points", "part_nodes", "part_first_code")}
    res["label_first"], res["label_largest"], res["n_parts"] = out["label_first"], out["label_largest"][:k], c
    res["map"] = [out["map"][int(p_off[r]):int(p_off[r + 1])] for r in range(world)]
    return res


def _label_graph_fields():
    from .api import Engine
    return Engine.LABEL_GRAPH_FIELDS


def fold_label_edges(records, K):
    """vgs_tiles_fold_label_edges (host arithmetic, no GPU): step 6 of vgs_tiles_point_label_graph.  records[r] = rank r's partial table
    as a dict of the fields of Engine.label_graph() -- what NativeTiles.own_point_label_graph() gives.  Returns the folded table in the
    same form, with n_edges."""
    fields = _label_graph_fields()
    world, K = len(records), int(K)
    off = np.zeros(world + 1, dtype=np.int64)
    off[1:] = np.cumsum([np.asarray(r["seg_ab"]).reshape(-1, 2).shape[0] for r in records])
    ins = [np.ascontiguousarray(np.concatenate([np.asarray(r[name], dtype=dt).reshape(-1) for r in records] + [np.zeros(0, dtype=dt)])) for name, dt, _ in fields]
    R = max(int(off[-1]), 1)
    out = {name: np.zeros((R, w) if w > 1 else R, dtype=dt) for name, dt, w in fields}
    E = C.c_int64(0)
    st = lib().vgs_tiles_fold_label_edges(world, K, _vp(off), *(_vp(a) for a in ins), C.byref(E), *(_vp(out[name]) for name, _, _ in fields))
    if st != 0:
        raise VgsError(st, "vgs_tiles_fold_label_edges")
    res = {name: out[name][:E.value] for name, _, _ in fields}
    res["n_edges"] = int(E.value)
    return res


def _rec_off(records):
    off = np.zeros(len(records) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r["label"]) for r in records])
    return off


def fold_field_moments(records, K, n_channels):
    """vgs_tiles_fold_field_moments (host arithmetic, no GPU): records[r] = rank r's dict of label (int32) and FIELD_MOMENT_FIELDS arrays
    (records x n_channels), as vgs_get_own_segment_field_moments gives them; returns the K folded rows as a dict of FIELD_MOMENT_FIELDS
    arrays (K, n_channels)."""
    K, ch = int(K), int(n_channels)
    off = _rec_off(records)
    lab = np.ascontiguousarray(np.concatenate([np.asarray(r["label"]) for r in records]).astype(np.int32))
    flat = {name: np.ascontiguousarray(np.concatenate([np.asarray(r[name], dtype=dt).reshape(-1, max(ch, 1)) for r in records]).reshape(-1))
            for name, dt in FIELD_MOMENT_FIELDS}
    out = {name: np.zeros((max(K, 1), max(ch, 1)), dtype=dt) for name, dt in FIELD_MOMENT_FIELDS}
    st = lib().vgs_tiles_fold_field_moments(len(records), _vp(off), _vp(lab), ch, *(_vp(flat[name]) for name, _ in FIELD_MOMENT_FIELDS), K,
                                            *(_vp(out[name]) for name, _ in FIELD_MOMENT_FIELDS))
    if st != 0:
        raise VgsError(st, "vgs_tiles_fold_field_moments")
    return {name: a[:max(K, 0)] for name, a in out.items()}


def fold_class_counts(records, K, n_classes):
    """vgs_tiles_fold_class_counts (host arithmetic, no GPU): records[r] = rank r's dict of label (int32), hist (records x n_classes, int64)
    and n_outside (int64), as vgs_get_own_segment_class_counts gives them; returns the dict of Engine.segment_class_histogram()."""
    from .api import Engine
    K, nc = int(K), int(n_classes)
    off = _rec_off(records)
    lab = np.ascontiguousarray(np.concatenate([np.asarray(r["label"]) for r in records]).astype(np.int32))
    hist = np.ascontiguousarray(np.concatenate([np.asarray(r["hist"], dtype=np.int64).reshape(-1, max(nc, 1)) for r in records]).reshape(-1))
    nout = np.ascontiguousarray(np.concatenate([np.asarray(r["n_outside"], dtype=np.int64).reshape(-1) for r in records]))
    out = {name: np.zeros((max(K, 1), max(nc, 1)) if w == 0 else max(K, 1), dtype=dt) for name, dt, w in Engine.CLASS_HIST_FIELDS}
    st = lib().vgs_tiles_fold_class_counts(len(records), _vp(off), _vp(lab), nc, _vp(hist), _vp(nout), K,
                                           *(_vp(out[name]) for name, _, _ in Engine.CLASS_HIST_FIELDS))
    if st != 0:
        raise VgsError(st, "vgs_tiles_fold_class_counts")
    return {name: a[:max(K, 0)] for name, a in out.items()}


# ---- RCCL through ctypes: the three calls a caller needs to hand the driver a communicator ---------------------------------------
class _NcclUniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


def rccl():
    global _RCCL
    if _RCCL is None:
        R = C.CDLL("librccl.so.1" if os.path.exists("/opt/rocm/lib/librccl.so.1") else "librccl.so")
        R.ncclGetUniqueId.restype = C.c_int
        R.ncclGetUniqueId.argtypes = [C.POINTER(_NcclUniqueId)]
        R.ncclCommInitRank.restype = C.c_int
        R.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, _NcclUniqueId, C.c_int]   # the id travels BY VALUE
        R.ncclCommCount.restype = C.c_int
        R.ncclCommCount.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        R.ncclCommDestroy.restype = C.c_int
        R.ncclCommDestroy.argtypes = [C.c_void_p]
        R.ncclCommAbort.restype = C.c_int
        R.ncclCommAbort.argtypes = [C.c_void_p]
        R.ncclGetErrorString.restype = C.c_char_p
        R.ncclGetErrorString.argtypes = [C.c_int]
        _RCCL = R
    return _RCCL


def rccl_unique_id() -> bytes:
    """rank 0: a fresh ncclUniqueId (128 bytes) to hand to the other ranks"""
    uid = _NcclUniqueId()
    st = rccl().ncclGetUniqueId(C.byref(uid))
    if st != 0:
        raise RuntimeError(f"ncclGetUniqueId: {rccl().ncclGetErrorString(st).decode()}")
    return bytes(C.string_at(C.byref(uid), 128))


class RcclComm:
    """An ncclComm_t owned by this process (the HIP device must be the current one: hipSetDevice before the call)."""

    def __init__(self, uid: bytes, rank: int, world: int, device: int):
        hip = C.CDLL("libamdhip64.so")
        if hip.hipSetDevice(int(device)) != 0:
            raise RuntimeError(f"hipSetDevice({device}) failed")
        u = _NcclUniqueId()
        C.memmove(C.byref(u), uid, 128)
        self.handle = C.c_void_p()
        st = rccl().ncclCommInitRank(C.byref(self.handle), int(world), u, int(rank))
        if st != 0:
            raise RuntimeError(f"ncclCommInitRank(rank {rank} of {world}): {rccl().ncclGetErrorString(st).decode()}")
        self.rank, self.world = rank, world

    def count(self) -> int:
        n = C.c_int(0)
        st = rccl().ncclCommCount(self.handle, C.byref(n))
        if st != 0:
            raise RuntimeError(f"ncclCommCount: {rccl().ncclGetErrorString(st).decode()}")
        return n.value

    def destroy(self):
        if self.handle and self.handle.value:
            rccl().ncclCommDestroy(self.handle)
            self.handle = C.c_void_p()

    def abort(self):
        if self.handle and self.handle.value:
            rccl().ncclCommAbort(self.handle)
            self.handle = C.c_void_p()


class LocalGroup:
    """`world` driver threads of one process meeting in shared memory (tests: several ranks on one GPU)."""

    def __init__(self, world):
        self.handle = C.c_void_p()
        st = lib().vgs_tiles_local_group_create(int(world), C.byref(self.handle))
        if st != 0:
            raise VgsError(st, "vgs_tiles_local_group_create")

    def abort(self):
        lib().vgs_tiles_local_group_abort(self.handle)

    def close(self):
        if self.handle and self.handle.value:
            lib().vgs_tiles_local_group_destroy(self.handle)
            self.handle = C.c_void_p()


class NativeTiles:
    """One rank of the native tiled driver."""

    def __init__(self, params: VgsParams, comm_kind: int, comm_handle, rank: int, world: int, tiles, pitch: float, center=(0.0, 0.0), keep=None):
        self._L = lib()
        self._h = C.c_void_p()
        self._keep = keep          # whatever the communicator handle points into (callback thunks, comm objects)
        self.rank, self.world = rank, world
        self.params = params
        st = self._L.vgs_tiles_create(C.byref(params), comm_kind, comm_handle, rank, world, int(tiles[0]), int(tiles[1]), float(pitch),
                                      float(center[0]), float(center[1]), C.byref(self._h))
        if st != 0:
            raise VgsError(st, f"vgs_tiles_create: {_lib.lib().vgs_last_error_string(None).decode()}")
        self.n = 0

    @classmethod
    def with_callbacks(cls, params, rank, world, tiles, pitch, all_gather, bcast, center=(0.0, 0.0)):
        """all_gather(send: bytes-like numpy uint8 view, recv: numpy uint8 view of world * n bytes) and bcast(buf: numpy uint8 view,
        root) are the caller's transport over host memory; exceptions they raise become a failed collective (VGS_E_HIP)."""
        def _ag(user, send, recv, nbytes):
            try:
                s = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(int(nbytes),))
                r = np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(int(nbytes) * world,))
                all_gather(s, r)
                return 0
            except Exception as ex:  # noqa: BLE001 (the C side turns this into an error status; the message goes to stderr)
                import sys
                print(f"[tiles_native] all_gather callback failed: {ex!r}", file=sys.stderr)
                return 1

        def _bc(user, buf, nbytes, root):
            try:
                b = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), shape=(int(nbytes),))
                bcast(b, int(root))
                return 0
            except Exception as ex:  # noqa: BLE001
                import sys
                print(f"[tiles_native] bcast callback failed: {ex!r}", file=sys.stderr)
                return 1

        cb = _Callbacks(None, _AG_FN(_ag), _BC_FN(_bc))
        return cls(params, COMM_CALLBACKS, C.cast(C.pointer(cb), C.c_void_p), rank, world, tiles, pitch, center, keep=cb)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.vgs_tiles_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        if st != 0:
            raise VgsError(st, self._L.vgs_tiles_last_error_string(self._h).decode())

    def set_option(self, option, value):
        self._ck(self._L.vgs_tiles_set_option(self._h, int(option), int(value)))

    def set_points(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
            raise ValueError("xyz must be (N,3) or (N,4) float32")
        self._xyz = xyz
        self.n = xyz.shape[0]
        self._ck(self._L.vgs_tiles_set_points(self._h, xyz.ctypes.data_as(C.c_void_p), xyz.shape[0], xyz.shape[1] * 4))

    def run(self):
        self._ck(self._L.vgs_tiles_run(self._h))

    def _times(self, getter, names):
        """one of the driver's phase clocks on this rank: name -> milliseconds of host wall time"""
        t = np.zeros(len(names), dtype=np.float64)
        self._ck(getter(self._h, _vp(t), len(names)))
        return dict(zip(names, (float(x) for x in t)))

    def _payload(self, getter, names):
        """one of the driver's payload counters on this rank: name -> int64"""
        v = [C.c_int64(0) for _ in names]
        self._ck(getter(self._h, *(C.byref(x) for x in v)))
        return dict(zip(names, (x.value for x in v)))

    def times(self):
        return self._times(self._L.vgs_tiles_get_times, T_NAMES)

    def point_labels(self):
        out = np.zeros(max(self.n, 1), dtype=np.int32)
        kept = C.c_int64(0)
        self._ck(self._L.vgs_tiles_get_point_labels(self._h, out.ctypes.data_as(C.c_void_p), C.byref(kept)))
        return out[:self.n], int(kept.value)

    def segment_descriptors(self):
        """COLLECTIVE (every rank calls it after run()): the descriptors of the global segments over all ranks, row k = the points
        point_labels() labels k on any rank -- the dict of Engine.segment_descriptors(), the same bytes on every rank
        (include/vgs_tiles.h, vgs_tiles_get_segment_descriptors).  Cached until the next run() or set_points()."""
        from .api import Engine
        K = C.c_int64(0)
        self._ck(self._L.vgs_tiles_get_segment_descriptors(self._h, C.byref(K), *([None] * len(Engine.DESCRIPTOR_FIELDS))))
        k = int(K.value)
        out = {name: np.zeros((k, w) if w > 1 else k, dtype=dt) for name, dt, w in Engine.DESCRIPTOR_FIELDS}
        if k == 0:
            return out
        self._ck(self._L.vgs_tiles_get_segment_descriptors(self._h, C.byref(K), *(_vp(out[name]) for name, _, _ in Engine.DESCRIPTOR_FIELDS)))
        return out

    def descriptor_times(self):
        """the last descriptor collective's phases on this rank, milliseconds (D_NAMES)"""
        return self._times(self._L.vgs_tiles_get_descriptor_times, D_NAMES)

    def segment_graph(self):
        """COLLECTIVE on its first call after run() (every rank makes it): the adjacency graph of the global segments over all ranks,
        labels = point_labels() on any rank -- the dict of Engine.segment_graph(), the same bytes on every rank (include/vgs_tiles.h,
        vgs_tiles_get_segment_graph).  Cached until the next run() or set_points(): later calls make no collective."""
        F = _graph_fields()
        E = C.c_int64(0)
        self._ck(self._L.vgs_tiles_get_segment_graph(self._h, C.byref(E), *([None] * len(F))))
        out = {name: np.zeros((E.value, w) if w > 1 else E.value, dtype=dt) for name, dt, w in F}
        if E.value:
            self._ck(self._L.vgs_tiles_get_segment_graph(self._h, C.byref(E), *(_vp(out[name]) for name, _, _ in F)))
        return out

    def graph_times(self):
        """the last graph collective's phases on this rank, milliseconds (G_NAMES)"""
        return self._times(self._L.vgs_tiles_get_graph_times, G_NAMES)

    def graph_payload(self):
        """the last graph collective's payload on this rank: halo labels handed to the context, edges of its own table, bytes sent"""
        return self._payload(self._L.vgs_tiles_get_graph_payload, ("halo_labels", "own_edges", "bytes_sent"))

    def own_segment_graph(self, K):
        """this rank's partial edge table over the global labels 0 .. K-1 (vgs_get_own_segment_graph on its context; local, no
        collective; the halo labels are those of the last segment_graph() collective, if any)"""
        L = _lib.lib()
        h = self._ctx()
        F = _graph_fields()
        E = C.c_int64(0)
        st = L.vgs_get_own_segment_graph(h, int(K), C.byref(E), *([None] * len(F)))
        out = {name: np.zeros((E.value, w) if w > 1 else E.value, dtype=dt) for name, dt, w in F}
        if st == 0 and E.value:
            st = L.vgs_get_own_segment_graph(h, int(K), C.byref(E), *(_vp(out[name]) for name, _, _ in F))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        return out

    def segment_boxes(self, frame="principal"):
        """COLLECTIVE while this frame's table is not cached (every rank calls it after run()): the oriented boxes of the global segments
        over all ranks, row k = the points point_labels() labels k on any rank -- the dict of Engine.segment_boxes(frame), the same
        bytes on every rank (include/vgs_tiles.h, vgs_tiles_get_segment_boxes).  Takes the descriptor table first (its collective, unless
        it is cached).  Cached per frame until the next run() or set_points(): later calls make no collective."""
        from .api import Engine
        f = int(Engine.BOX_FRAMES.get(frame, frame))
        K = C.c_int64(0)
        self._ck(self._L.vgs_tiles_get_segment_boxes(self._h, f, C.byref(K), *([None] * len(Engine.BOX_FIELDS))))
        k = int(K.value)
        out = {name: np.zeros((max(k, 1), w), dtype=dt) for name, dt, w in Engine.BOX_FIELDS}   # (K = 0 still makes the call: its status, its collective)
        self._ck(self._L.vgs_tiles_get_segment_boxes(self._h, f, C.byref(K), *(_vp(out[name]) for name, _, _ in Engine.BOX_FIELDS)))
        return {name: a[:k] for name, a in out.items()}

    def box_times(self):
        """the last box collective's phases on this rank, milliseconds (B_NAMES)"""
        return self._times(self._L.vgs_tiles_get_box_times, B_NAMES)

    def own_segment_extents(self, K, frame, d):
        """this rank's extent records of the global labels 0 .. K-1 (vgs_get_own_segment_extents on its context; local, no collective)
        about the centroid3 / cov6 / evecs9 rows of the global descriptor table d: a dict of label, lo3, hi3"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        K = int(K)
        rows = [np.ascontiguousarray(np.asarray(d[name], dtype=np.float64).reshape(-1)) for name in ("centroid3", "cov6", "evecs9")]
        out = {"label": np.zeros(max(K, 1), dtype=np.int32), "lo3": np.zeros((max(K, 1), 3)), "hi3": np.zeros((max(K, 1), 3))}
        n = C.c_int64(0)
        st = L.vgs_get_own_segment_extents(h, K, int(Engine.BOX_FRAMES.get(frame, frame)), *(_vp(a) for a in rows), C.byref(n),
                                           _vp(out["label"]), _vp(out["lo3"]), _vp(out["hi3"]))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        return {name: a[:n.value] for name, a in out.items()}

    def segment_field_stats(self, field):
        """COLLECTIVE on every call (every rank makes it after run(), with the same number of channels; nothing is cached): the statistics
        of a per-point attribute over the global segments, row k = the points point_labels() labels k on any rank -- the dict of
        Engine.segment_field_stats(), the same bytes on every rank (include/vgs_tiles.h, vgs_tiles_segment_field_stats).  `field`: one row
        per point of this rank's set_points(), float32 (N,) or (N, C) with the stride rules of Engine.segment_field_stats; a numpy array,
        or a torch tensor on this rank's device, which is read in place.  No attribute leaves the rank, only per-segment records."""
        from .api import Engine
        field, ptr, n, ch, stride, dev = Engine._field_input(field, self.params.device)
        fn = self._L.vgs_tiles_segment_field_stats_device if dev else self._L.vgs_tiles_segment_field_stats
        K = C.c_int64(0)
        k = self._kept()
        out = {name: np.zeros((max(k, 1), max(ch, 1)), dtype=dt) for name, dt in Engine.FIELD_STAT_FIELDS}
        self._ck(fn(self._h, ptr, n, ch, stride, C.byref(K), *(_vp(out[name]) for name, _ in Engine.FIELD_STAT_FIELDS)))
        return {name: a[:k, :max(ch, 0)] for name, a in out.items()}

    def segment_class_histogram(self, classes, n_classes):
        """COLLECTIVE on every call (every rank makes it after run(), with the same n_classes; nothing is cached): the class histogram of
        the global segments over all ranks -- the dict of Engine.segment_class_histogram(), the same bytes on every rank
        (include/vgs_tiles.h, vgs_tiles_segment_class_histogram).  `classes`: one int32 per point of this rank's set_points(), numpy or a
        torch tensor on this rank's device."""
        from .api import Engine
        nc = int(n_classes)
        classes, ptr, n, dev = Engine._classes_input(classes, self.params.device)
        fn = self._L.vgs_tiles_segment_class_histogram_device if dev else self._L.vgs_tiles_segment_class_histogram
        k = self._kept()
        w1 = max(nc, 1) if nc <= 1024 else 1
        out = {name: np.zeros((max(k, 1), w1) if w == 0 else max(k, 1), dtype=dt) for name, dt, w in Engine.CLASS_HIST_FIELDS}
        K = C.c_int64(0)
        self._ck(fn(self._h, ptr, n, nc, C.byref(K), *(_vp(out[name]) for name, _, _ in Engine.CLASS_HIST_FIELDS)))
        return {name: (a[:k, :max(nc, 0)] if a.ndim == 2 else a[:k]) for name, a in out.items()}

    def describe_labels(self, labels, K):
        """COLLECTIVE on every call (every rank makes it after run(), with the same K; nothing is cached): descriptors of ANY per-point
        labelling over all ranks -- the dict of Engine.describe_labels() on the gathered points, K rows plus n_skipped, the same bytes on
        every rank (include/vgs_tiles.h, vgs_tiles_point_label_descriptors).  `labels`: one int32 per point of this rank's set_points(),
        negative = no segment, a label >= K is an error; a numpy array, or a torch tensor on this rank's device, which is read in place.
        No point and no label leaves the rank, only per-label records."""
        from .api import Engine
        labels, ptr, n, dev = Engine._classes_input(labels, self.params.device)
        fn = self._L.vgs_tiles_point_label_descriptors_device if dev else self._L.vgs_tiles_point_label_descriptors
        K = int(K)
        k = K if 0 <= K <= 0x7fffffff else 0
        out = {name: np.zeros((max(k, 1), w) if w > 1 else max(k, 1), dtype=dt) for name, dt, w in Engine.DESCRIPTOR_FIELDS}
        skipped = C.c_int64(0)
        self._ck(fn(self._h, ptr, n, K, C.byref(skipped), *(_vp(out[name]) for name, _, _ in Engine.DESCRIPTOR_FIELDS)))
        out = {name: a[:k] for name, a in out.items()}
        out["n_skipped"] = int(skipped.value)
        return out

    def label_boxes(self, labels, frame, K):
        """COLLECTIVE on every call, two collectives (every rank makes it after run(), with the same K and frame; nothing is cached):
        oriented boxes of ANY per-point labelling over all ranks -- the dict of Engine.label_boxes() on the gathered points, the same
        bytes on every rank (include/vgs_tiles.h, vgs_tiles_point_label_boxes).  `labels`, K as describe_labels()."""
        from .api import Engine
        labels, ptr, n, dev = Engine._classes_input(labels, self.params.device)
        fn = self._L.vgs_tiles_point_label_boxes_device if dev else self._L.vgs_tiles_point_label_boxes
        K = int(K)
        k = K if 0 <= K <= 0x7fffffff else 0
        out = {name: np.zeros((max(k, 1), w), dtype=dt) for name, dt, w in Engine.BOX_FIELDS}
        self._ck(fn(self._h, ptr, n, K, int(Engine.BOX_FRAMES.get(frame, frame)), *(_vp(out[name]) for name, _, _ in Engine.BOX_FIELDS)))
        return {name: a[:k] for name, a in out.items()}

    def point_label_times(self):
        """the last describe_labels() / label_boxes()'s phases on this rank, milliseconds (L_NAMES; label_boxes: both collectives added)"""
        return self._times(self._L.vgs_tiles_get_point_label_times, L_NAMES)

    def point_label_payload(self):
        """the last describe_labels() / label_boxes()'s payload on this rank: moment records and pair records of its own, bytes sent"""
        return self._payload(self._L.vgs_tiles_get_point_label_payload, ("own_records", "own_pairs", "bytes_sent"))

    def own_point_label_moments(self, K, labels):
        """this rank's moment and pair records of a labelling of its own points (vgs_own_point_label_moments on its context; local, no
        collective): a dict of label and MOMENT_FIELDS arrays (one row per label with an own finite point), pair_code (uint64) and
        pair_label (int32) -- the head flags in voxels that hold another rank's points too --, plus n_skipped"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        labels, ptr, n, dev = Engine._classes_input(labels, self.params.device)
        fn = L.vgs_own_point_label_moments_device if dev else L.vgs_own_point_label_moments
        nr, npair, nskip = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        st = fn(h, int(K), ptr, n, C.byref(nr), C.byref(npair), C.byref(nskip))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {"label": np.zeros(max(nr.value, 1), dtype=np.int32)}
        for name, dt, w in MOMENT_FIELDS:
            out[name] = np.zeros((max(nr.value, 1), w) if w > 1 else max(nr.value, 1), dtype=dt)
        pc, pl = np.zeros(max(npair.value, 1), dtype=np.uint64), np.zeros(max(npair.value, 1), dtype=np.int32)
        st = L.vgs_get_own_point_label_moments(h, _vp(out["label"]), *(_vp(out[name]) for name, _, _ in MOMENT_FIELDS), _vp(pc), _vp(pl))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {name: a[:nr.value] for name, a in out.items()}
        out["pair_code"], out["pair_label"], out["n_skipped"] = pc[:npair.value], pl[:npair.value], int(nskip.value)
        return out

    def label_components(self, labels, K):
        """COLLECTIVE on every call, two collectives (every rank makes it after run(), with the same K; nothing is cached): the connected
        parts of ANY per-point labelling over all ranks -- the dict of Engine.label_components() on the gathered points, with
        part_first_code (uint64, the shared-grid code of the part's first node) in place of part_first_node; part_of_point holds this
        rank's points, every table the same bytes on every rank (include/vgs_tiles.h, vgs_tiles_point_label_components).  `labels`, K as
        describe_labels().  The result stays in the driver until the next call, the next run or the next set_points()."""
        from .api import Engine
        labels, ptr, n, dev = Engine._classes_input(labels, self.params.device)
        fn = self._L.vgs_tiles_point_label_components_device if dev else self._L.vgs_tiles_point_label_components
        K = int(K)
        n_parts, skipped = C.c_int64(0), C.c_int64(0)
        self._ck(fn(self._h, ptr, n, K, C.byref(n_parts), C.byref(skipped)))
        out = self.label_components_result(n_parts.value, K)
        out["n_skipped"] = int(skipped.value)
        return out

    def label_components_result(self, n_parts, K):
        """the tables of the last label_components() (vgs_tiles_get_point_label_components; local, no collective)"""
        rows = {"points": self.n, "parts": int(n_parts), "first": max(int(K), 0) + 1, "labels": max(int(K), 0)}
        out = {name: np.zeros(max(rows[tab], 1), dtype=dt) for name, dt, tab in COMPONENT_FIELDS}
        self._ck(self._L.vgs_tiles_get_point_label_components(self._h, *(_vp(out[name]) for name, _, _ in COMPONENT_FIELDS)))
        out = {name: out[name][:rows[tab]] for name, _, tab in COMPONENT_FIELDS}
        out["n_parts"] = int(n_parts)
        return out

    def label_component_times(self):
        """the last label_components()'s phases on this rank, milliseconds (CC_NAMES)"""
        return self._times(self._L.vgs_tiles_get_point_label_component_times, CC_NAMES)

    def label_component_payload(self):
        """the last label_components()'s payload on this rank: band records, local parts and links of its own, bytes sent"""
        return self._payload(self._L.vgs_tiles_get_point_label_component_payload, ("band_records", "parts", "links", "bytes_sent"))

    def own_point_label_parts(self, labels, K):
        """this rank's local parts and band records of a labelling of its own points (vgs_own_point_label_parts on its context; local, no
        collective): a dict of part_label, part_points, part_nodes, part_first_code (one row per local part), band_code, band_label,
        band_part (one row per band vertex), plus n_skipped"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        labels, ptr, n, dev = Engine._classes_input(labels, self.params.device)
        fn = L.vgs_own_point_label_parts_device if dev else L.vgs_own_point_label_parts
        npart, nband, nskip = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        st = fn(h, ptr, n, int(K), C.byref(npart), C.byref(nband), C.byref(nskip))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        fields = (("part_label", np.int32, npart.value), ("part_points", np.int64, npart.value), ("part_nodes", np.int32, npart.value),
                  ("part_first_code", np.uint64, npart.value), ("band_code", np.uint64, nband.value), ("band_label", np.int32, nband.value),
                  ("band_part", np.int32, nband.value))
        out = {name: np.zeros(max(m, 1), dtype=dt) for name, dt, m in fields}
        st = L.vgs_get_own_point_label_parts(h, *(_vp(out[name]) for name, _, _ in fields))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {name: out[name][:m] for name, _, m in fields}
        out["n_skipped"] = int(nskip.value)
        return out

    def link_point_label_parts(self, code, label, rank, part):
        """this rank's cross links over other ranks' band records (vgs_link_point_label_parts behind own_point_label_parts(); local, no
        collective): a dict of link_own, link_rank, link_part (int32), sorted and unique"""
        L = _lib.lib()
        h = self._ctx()
        code = np.ascontiguousarray(code, dtype=np.uint64)
        label, rank, part = (np.ascontiguousarray(a, dtype=np.int32) for a in (label, rank, part))
        nl = C.c_int64(0)
        st = L.vgs_link_point_label_parts(h, _vp(code), _vp(label), _vp(rank), _vp(part), int(code.shape[0]), C.byref(nl))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {name: np.zeros(max(nl.value, 1), dtype=np.int32) for name in ("link_own", "link_rank", "link_part")}
        st = L.vgs_get_point_label_part_links(h, *(_vp(a) for a in out.values()))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        return {name: a[:nl.value] for name, a in out.items()}

    def label_graph(self, labels, K):
        """COLLECTIVE on every call, two collectives (every rank makes it after run(), with the same K; nothing is cached): the adjacency
        graph of ANY per-point labelling over all ranks -- the dict of Engine.label_graph() on the gathered points, the same bytes on every
        rank, w_sum summed over the ranks' partial sums in rank order (include/vgs_tiles.h, vgs_tiles_point_label_graph).  `labels`, K as
        label_components().  The table stays in the driver until the next call, the next run or the next set_points()."""
        from .api import Engine
        labels, ptr, n, dev = Engine._classes_input(labels, self.params.device)
        fn = self._L.vgs_tiles_point_label_graph_device if dev else self._L.vgs_tiles_point_label_graph
        E, skipped = C.c_int64(0), C.c_int64(0)
        self._ck(fn(self._h, ptr, n, int(K), C.byref(E), C.byref(skipped)))
        out = self.label_graph_result(E.value)
        out["n_skipped"] = int(skipped.value)
        return out

    def label_graph_result(self, n_edges):
        """the table of the last label_graph() (vgs_tiles_get_point_label_graph; local, no collective)"""
        E = int(n_edges)
        fields = _label_graph_fields()
        buf = {name: np.zeros((max(E, 1), w) if w > 1 else max(E, 1), dtype=dt) for name, dt, w in fields}
        self._ck(self._L.vgs_tiles_get_point_label_graph(self._h, *(_vp(buf[name]) for name, _, _ in fields)))
        out = {name: buf[name][:E] for name, _, _ in fields}
        out["n_edges"] = E
        return out

    def label_graph_times(self):
        """the last label_graph()'s phases on this rank, milliseconds (LG_NAMES)"""
        return self._times(self._L.vgs_tiles_get_label_graph_times, LG_NAMES)

    def label_graph_payload(self):
        """the last label_graph()'s payload on this rank: band records of its own, other ranks' records found in its grid, edges of its
        partial table, bytes sent"""
        return self._payload(self._L.vgs_tiles_get_label_graph_payload, ("band_records", "foreign_hits", "own_edges", "bytes_sent"))

    def own_point_label_band(self, labels, K):
        """this rank's band records of a labelling of its own points (vgs_own_point_label_band on its context; local, no collective): a
        dict of band_code (uint64), band_label (int32) and n_skipped"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        labels, ptr, n, dev = Engine._classes_input(labels, self.params.device)
        fn = L.vgs_own_point_label_band_device if dev else L.vgs_own_point_label_band
        nband, nskip = C.c_int64(0), C.c_int64(0)
        st = fn(h, ptr, n, int(K), C.byref(nband), C.byref(nskip))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        code, lab = np.zeros(max(nband.value, 1), dtype=np.uint64), np.zeros(max(nband.value, 1), dtype=np.int32)
        st = L.vgs_get_own_point_label_band(h, _vp(code), _vp(lab))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        return dict(band_code=code[:nband.value], band_label=lab[:nband.value], n_skipped=int(nskip.value))

    def own_point_label_graph(self, code, label):
        """this rank's partial table over other ranks' band records (vgs_own_point_label_graph behind own_point_label_band(); local, no
        collective): the dict of Engine.label_graph() without n_skipped"""
        L = _lib.lib()
        h = self._ctx()
        code = np.ascontiguousarray(code, dtype=np.uint64)
        label = np.ascontiguousarray(label, dtype=np.int32)
        E = C.c_int64(0)
        st = L.vgs_own_point_label_graph(h, _vp(code), _vp(label), int(code.shape[0]), C.byref(E))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        fields = _label_graph_fields()
        buf = {name: np.zeros((max(E.value, 1), w) if w > 1 else max(E.value, 1), dtype=dt) for name, dt, w in fields}
        st = L.vgs_get_own_point_label_graph(h, *(_vp(buf[name]) for name, _, _ in fields))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {name: buf[name][:E.value] for name, _, _ in fields}
        out["n_edges"] = int(E.value)
        return out

    def _label_table_inputs(self, labels, other, what):
        """labels of label_field_stats / label_class_histogram and the own-record calls: labels and the attribute array both numpy or both
        torch tensors on the rank's device -> (array kept alive, pointer, n, on the device?)"""
        from .api import Engine
        if Engine._is_torch(labels) != Engine._is_torch(other):
            raise ValueError(f"labels and {what} must both be numpy arrays or both be torch tensors on the rank's device")
        return Engine._classes_input(labels, self.params.device)

    def label_field_stats(self, labels, field, K):
        """COLLECTIVE on every call (every rank makes it after run(), with the same K and number of channels; nothing is cached): field
        statistics of ANY per-point labelling over all ranks -- the dict of Engine.label_field_stats() on the gathered points, K rows plus
        n_skipped (the sum over the ranks), the same bytes on every rank (include/vgs_tiles.h, vgs_tiles_point_label_field_stats).
        `labels` as describe_labels(), `field` as segment_field_stats(): one row per point of this rank's set_points(); both numpy arrays
        or both torch tensors on this rank's device, which are read in place.  No point, label or attribute leaves the rank, only
        per-label records."""
        from .api import Engine
        labels, lptr, ln, dev = self._label_table_inputs(labels, field, "field")
        field, ptr, n, ch, stride, _ = Engine._field_input(field, self.params.device)
        fn = self._L.vgs_tiles_point_label_field_stats_device if dev else self._L.vgs_tiles_point_label_field_stats
        K = int(K)
        k = K if 0 <= K <= 0x7fffffff and K * max(ch, 1) <= 1 << 27 else 0
        out = {name: np.zeros((max(k, 1), max(ch, 1)), dtype=dt) for name, dt in Engine.FIELD_STAT_FIELDS}
        skipped = C.c_int64(0)
        # (the library takes one n for both arrays: it is handed the length that is not this rank's, if one is not, so that it names it)
        self._ck(fn(self._h, lptr, K, ptr, ln if ln != self.n else n, ch, stride, C.byref(skipped), *(_vp(out[name]) for name, _ in Engine.FIELD_STAT_FIELDS)))
        out = {name: a[:k, :max(ch, 0)] for name, a in out.items()}
        out["n_skipped"] = int(skipped.value)
        return out

    def label_class_histogram(self, labels, classes, n_classes, K):
        """COLLECTIVE on every call (every rank makes it after run(), with the same K and n_classes; nothing is cached): the class
        histogram of ANY per-point labelling over all ranks -- the dict of Engine.label_class_histogram() on the gathered points, K rows
        plus n_skipped, the same bytes on every rank (include/vgs_tiles.h, vgs_tiles_point_label_class_histogram).  `labels` as
        describe_labels(), `classes` as segment_class_histogram(); both numpy arrays or both torch tensors on this rank's device."""
        from .api import Engine
        nc = int(n_classes)
        labels, lptr, ln, dev = self._label_table_inputs(labels, classes, "classes")
        classes, ptr, n, _ = Engine._classes_input(classes, self.params.device)
        fn = self._L.vgs_tiles_point_label_class_histogram_device if dev else self._L.vgs_tiles_point_label_class_histogram
        K = int(K)
        ok = 0 <= K <= 0x7fffffff and 1 <= nc <= 1024 and K * nc <= 1 << 27
        k, w1 = (K, nc) if ok else (0, 1)
        out = {name: np.zeros((max(k, 1), w1) if w == 0 else max(k, 1), dtype=dt) for name, dt, w in Engine.CLASS_HIST_FIELDS}
        skipped = C.c_int64(0)
        self._ck(fn(self._h, lptr, K, ptr, ln if ln != self.n else n, nc, C.byref(skipped), *(_vp(out[name]) for name, _, _ in Engine.CLASS_HIST_FIELDS)))
        out = {name: (a[:k, :nc if ok else 0] if a.ndim == 2 else a[:k]) for name, a in out.items()}
        out["n_skipped"] = int(skipped.value)
        return out

    def own_point_label_field_moments(self, K, labels, field):
        """this rank's attribute moments of a labelling of its own points (vgs_own_point_label_field_moments on its context; local, no
        collective): a dict of label and FIELD_MOMENT_FIELDS arrays (records, C), one record per label with an own point in the octree,
        plus n_skipped"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        K = int(K)
        labels, lptr, ln, dev = self._label_table_inputs(labels, field, "field")
        field, ptr, n, ch, stride, _ = Engine._field_input(field, self.params.device)
        fn = L.vgs_own_point_label_field_moments_device if dev else L.vgs_own_point_label_field_moments
        cap = min(K, max(ln, 0)) if 0 <= K <= 0x7fffffff else 0   # (one record per label with an own point)
        out = {"label": np.zeros(max(cap, 1), dtype=np.int32)}
        for name, dt in FIELD_MOMENT_FIELDS:
            out[name] = np.zeros((max(cap, 1), max(ch, 1)), dtype=dt)
        nr, nskip = C.c_int64(0), C.c_int64(0)
        st = fn(h, K, lptr, ptr, ln if ln != self.n else n, ch, stride, C.byref(nr), C.byref(nskip), _vp(out["label"]),
                *(_vp(out[name]) for name, _ in FIELD_MOMENT_FIELDS))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {name: a[:nr.value] for name, a in out.items()}
        out["n_skipped"] = int(nskip.value)
        return out

    def own_point_label_class_counts(self, K, labels, classes, n_classes):
        """this rank's class counts of a labelling of its own points (vgs_own_point_label_class_counts on its context; local, no
        collective): a dict of label, hist (records, n_classes) and n_outside, plus n_skipped"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        K, nc = int(K), int(n_classes)
        labels, lptr, ln, dev = self._label_table_inputs(labels, classes, "classes")
        classes, ptr, n, _ = Engine._classes_input(classes, self.params.device)
        fn = L.vgs_own_point_label_class_counts_device if dev else L.vgs_own_point_label_class_counts
        cap = min(K, max(ln, 0)) if 0 <= K <= 0x7fffffff else 0
        w1 = nc if 1 <= nc <= 1024 else 1
        out = {"label": np.zeros(max(cap, 1), dtype=np.int32), "hist": np.zeros((max(cap, 1), w1), dtype=np.int64),
               "n_outside": np.zeros(max(cap, 1), dtype=np.int64)}
        nr, nskip = C.c_int64(0), C.c_int64(0)
        st = fn(h, K, lptr, ptr, ln if ln != self.n else n, nc, C.byref(nr), C.byref(nskip), _vp(out["label"]), _vp(out["hist"]), _vp(out["n_outside"]))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {name: a[:nr.value] for name, a in out.items()}
        out["n_skipped"] = int(nskip.value)
        return out

    def compare_labels(self, ref, labels=None, K=None):
        """COLLECTIVE on every call (every rank makes it after run(); nothing is cached): score the segmentation against reference labels
        over all ranks -- the dict of Engine.compare_labels(), the same bytes on every rank, and what one engine gives on the gathered
        points (include/vgs_tiles.h, vgs_tiles_compare_labels).  `ref`: one int32 per point of this rank's set_points(), negative = not
        annotated; a numpy array, or a torch tensor on this rank's device, which is read in place.  No label and no id leaves the rank,
        only contingency cells; comparison_scores() works on the result unchanged.
        `labels` (vgs_tiles_compare_point_labels): score this labelling of the rank's points instead of point_labels() -- refined_labels(),
        say -- with K segment rows, the same K on every rank; negative = dropped, a label >= K is an error; numpy or a torch tensor on
        this rank's device, as `ref` is (both of one kind)."""
        from .api import Engine
        if labels is not None:
            if Engine._is_torch(ref) != Engine._is_torch(labels):
                raise ValueError("ref and labels must both be numpy arrays or both be torch tensors on the rank's device")
            if K is None:
                raise ValueError("K is required with labels")
            ref, ptr, n, dev = Engine._classes_input(ref, self.params.device)
            labels, lptr, ln, _ = Engine._classes_input(labels, self.params.device)
            if ln != n:
                raise ValueError("ref and labels must have the same length")
            fn = self._L.vgs_tiles_compare_point_labels_device if dev else self._L.vgs_tiles_compare_point_labels
            n_cells, n_refs = C.c_int64(0), C.c_int64(0)
            summary = np.zeros(12, np.int64)
            self._ck(fn(self._h, lptr, int(K), ptr, n, C.byref(n_cells), C.byref(n_refs), _vp(summary)))
            out = self.label_comparison(n_cells.value, n_refs.value, max(int(K), 0))
            out["summary"] = summary
            return out
        ref, ptr, n, dev = Engine._classes_input(ref, self.params.device)
        fn = self._L.vgs_tiles_compare_labels_device if dev else self._L.vgs_tiles_compare_labels
        K, n_cells, n_refs = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        summary = np.zeros(12, np.int64)
        self._ck(fn(self._h, ptr, n, C.byref(K), C.byref(n_cells), C.byref(n_refs), _vp(summary)))
        out = self.label_comparison(n_cells.value, n_refs.value, K.value)
        out["summary"] = summary
        return out

    def label_comparison(self, n_cells, n_refs, K):
        """the tables of the last compare_labels() of this rank (vgs_tiles_get_label_comparison; local, no collective), with the sizes
        that call returned; VgsError (VGS_E_STATE) without a compare since the last run() or set_points()"""
        from .api import Engine
        rows = {"cells": int(n_cells), "refs": int(n_refs), "segs": int(K)}
        out = {name: np.zeros(max(rows[tab], 1), dtype=dt) for name, dt, tab in Engine.COMPARE_FIELDS}
        self._ck(self._L.vgs_tiles_get_label_comparison(self._h, *(_vp(out[name]) for name, _, _ in Engine.COMPARE_FIELDS)))
        return {name: out[name][:rows[tab]] for name, _, tab in Engine.COMPARE_FIELDS}

    def compare_times(self):
        """the last compare_labels()'s phases on this rank, milliseconds (C_NAMES)"""
        return self._times(self._L.vgs_tiles_get_compare_times, C_NAMES)

    def compare_payload(self):
        """the last compare_labels()'s payload on this rank: cells of its own, bytes sent"""
        return self._payload(self._L.vgs_tiles_get_compare_payload, ("own_cells", "bytes_sent"))

    def own_label_cells(self, K, ref):
        """this rank's contingency cells of the global labels -1 .. K-1 over its own points (vgs_own_label_cells on its context; local, no
        collective; it discards the context's last comparison): a dict of cell_seg, cell_ref (int32), cell_n (int64), ascending
        (segment, id), plus n_unannotated"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        ref, ptr, n, dev = Engine._classes_input(ref, self.params.device)
        fn = L.vgs_own_label_cells_device if dev else L.vgs_own_label_cells
        nc, nu = C.c_int64(0), C.c_int64(0)
        st = fn(h, int(K), ptr, n, C.byref(nc), C.byref(nu))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {"cell_seg": np.zeros(max(nc.value, 1), np.int32), "cell_ref": np.zeros(max(nc.value, 1), np.int32),
               "cell_n": np.zeros(max(nc.value, 1), np.int64)}
        st = L.vgs_get_own_label_cells(h, _vp(out["cell_seg"]), _vp(out["cell_ref"]), _vp(out["cell_n"]))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        out = {name: a[:nc.value] for name, a in out.items()}
        out["n_unannotated"] = int(nu.value)
        return out

    def refine_labels(self, patch_radius=None, switch_ratio=None, fill=True):
        """COLLECTIVE on every call (every rank makes it after run(), with the same parameters): point-level label refinement over all
        ranks -- the rule of Engine.refine_labels() on the whole scene, every point evaluated by the rank that loaded it
        (include/vgs_tiles.h, vgs_tiles_refine_point_labels).  None: the context's default (patch_radius = voxel_size, switch_ratio =
        0.25).  A new output next to point_labels(), read with refined_labels(); returns this rank's share of the counts
        (REFINE_COUNTS), which add over the ranks."""
        rp = _lib.VgsRefineParams()
        st = _lib.lib().vgs_refine_params_default(self._ctx(), C.byref(rp))
        if st != 0:
            raise VgsError(st, "vgs_refine_params_default")
        if patch_radius is not None:
            rp.patch_radius = float(patch_radius)
        if switch_ratio is not None:
            rp.switch_ratio = float(switch_ratio)
        rp.fill = 1 if fill else 0
        cnt = np.zeros(5, dtype=np.int64)
        self._ck(self._L.vgs_tiles_refine_point_labels(self._h, C.byref(rp), _vp(cnt)))
        return {name: int(v) for name, v in zip(REFINE_COUNTS, cnt)}

    def refined_labels(self):
        """the labels of the last refine_labels(), one int32 per point of this rank's set_points() (local, no collective); VgsError
        (VGS_E_STATE) without a refine since the last run() or set_points()"""
        out = np.zeros(max(self.n, 1), dtype=np.int32)
        self._ck(self._L.vgs_tiles_get_refined_labels(self._h, _vp(out)))
        return out[:self.n]

    def refine_times(self):
        """the last refine_labels()'s phases on this rank, milliseconds (R_NAMES)"""
        return self._times(self._L.vgs_tiles_get_refine_times, R_NAMES)

    def refine_payload(self):
        """the last refine_labels()'s payload on this rank: band records it sent (0 after the first call of a run), bytes sent"""
        return self._payload(self._L.vgs_tiles_get_refine_payload, ("band_records", "bytes_sent"))

    def _kept(self):
        """kept_global of the last run (0 before one); local"""
        K = C.c_int64(0)
        self._L.vgs_tiles_get_segment_descriptors(self._h, C.byref(K), *([None] * 8))
        return int(K.value)

    def field_times(self):
        """the last attribute collective's phases on this rank, milliseconds (F_NAMES)"""
        return self._times(self._L.vgs_tiles_get_field_times, F_NAMES)

    def field_payload(self):
        """the last attribute collective's payload on this rank: records of its own, bytes sent"""
        return self._payload(self._L.vgs_tiles_get_field_payload, ("own_records", "bytes_sent"))

    def own_segment_field_moments(self, K, field):
        """this rank's attribute moments of the global labels 0 .. K-1 over its own rows (vgs_get_own_segment_field_moments on its context;
        local, no collective): a dict of label and FIELD_MOMENT_FIELDS arrays (records, C)"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        K = int(K)
        field, ptr, n, ch, stride, dev = Engine._field_input(field, self.params.device)
        fn = L.vgs_get_own_segment_field_moments_device if dev else L.vgs_get_own_segment_field_moments
        out = {"label": np.zeros(max(K, 1), dtype=np.int32)}
        for name, dt in FIELD_MOMENT_FIELDS:
            out[name] = np.zeros((max(K, 1), max(ch, 1)), dtype=dt)
        nr = C.c_int64(0)
        st = fn(h, K, ptr, n, ch, stride, C.byref(nr), _vp(out["label"]), *(_vp(out[name]) for name, _ in FIELD_MOMENT_FIELDS))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        return {name: a[:nr.value] for name, a in out.items()}

    def own_segment_class_counts(self, K, classes, n_classes):
        """this rank's class counts of the global labels 0 .. K-1 over its own rows (vgs_get_own_segment_class_counts on its context; local,
        no collective): a dict of label, hist (records, n_classes) and n_outside"""
        from .api import Engine
        L = _lib.lib()
        h = self._ctx()
        K, nc = int(K), int(n_classes)
        classes, ptr, n, dev = Engine._classes_input(classes, self.params.device)
        fn = L.vgs_get_own_segment_class_counts_device if dev else L.vgs_get_own_segment_class_counts
        out = {"label": np.zeros(max(K, 1), dtype=np.int32), "hist": np.zeros((max(K, 1), max(nc, 1)), dtype=np.int64),
               "n_outside": np.zeros(max(K, 1), dtype=np.int64)}
        nr = C.c_int64(0)
        st = fn(h, K, ptr, n, nc, C.byref(nr), _vp(out["label"]), _vp(out["hist"]), _vp(out["n_outside"]))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        return {name: a[:nr.value] for name, a in out.items()}

    def own_segment_moments(self, K):
        """this rank's moment records of the global labels 0 .. K-1 (vgs_get_own_segment_moments on its context; local, no collective):
        a dict of MOMENT_FIELDS arrays plus label"""
        L = _lib.lib()
        h = self._ctx()
        K = int(K)
        out = {"label": np.zeros(max(K, 1), dtype=np.int32)}
        for name, dt, w in MOMENT_FIELDS:
            out[name] = np.zeros((max(K, 1), w) if w > 1 else max(K, 1), dtype=dt)
        n = C.c_int64(0)
        st = L.vgs_get_own_segment_moments(h, K, C.byref(n), _vp(out["label"]), *(_vp(out[name]) for name, _, _ in MOMENT_FIELDS))
        if st != 0:
            raise VgsError(st, L.vgs_last_error_string(h).decode())
        return {name: a[:n.value] for name, a in out.items()}

    def info(self):
        return self._payload(self._L.vgs_tiles_get_info, ("n_outside", "n_local", "n_boundary_records"))

    def exchange(self):
        """the last run's boundary exchange: bytes this rank sent / received, collectives taken"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._ck(self._L.vgs_tiles_get_exchange(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(bytes_sent=a.value, bytes_received=b.value, collectives=c.value)

    def bbox(self):
        from .api import Engine
        return Engine.bbox(_CtxView(self._ctx()))

    # read-only views of the rank's engine context (counts, stage times)
    def _ctx(self):
        return C.c_void_p(self._L.vgs_tiles_context(self._h))

    def counts(self):
        from .api import Engine
        return Engine.counts(_CtxView(self._ctx()))

    def stage_times(self):
        from .api import Engine
        return Engine.stage_times(_CtxView(self._ctx()))


class _CtxView:
    """Just enough of an Engine for its read-only getters, over a context the native driver owns."""

    def __init__(self, h):
        self._L = _lib.lib()
        self._h = h

    def _ck(self, st):
        if st != _lib.VGS_OK:
            raise VgsError(st, self._L.vgs_last_error_string(self._h).decode())
