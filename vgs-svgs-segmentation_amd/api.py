"""Host-side mirror of the reference's class API over the C-ABI (include/vgs.h).

`Engine` is a thin handle wrapper (one method per C entry point, numpy in/out).
`VoxelBasedSegmentation` / `SuperVoxelBasedSegmentation` keep the reference's method names, argument
meaning and call order (voxel_segmentation.h:84-421, 947-1014; supervoxel_segmentation.h:85-421), so the
driver snippets of the reference's `test` file (test:51-76, test:138-160) read the same here.
The C++ twin of this file is include/vgs_segmentation.hpp.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import VgsError, VgsGridState, VgsParams, VgsRefineParams


def comparison_scores(cmp, tau=0.5):
    """Scores of a label comparison (the dict of Engine.compare_labels, or tests/label_compare_ref.py's restatement), a pure function:
      matched       segments whose best id overlaps them with IoU > tau.  For tau >= 0.5 a segment matches at most one id and an id at most
                    one segment, so the same number comes out of ref_best_iou
      precision     matched / segments with an annotated point (summary[5]);  recall  matched / G;  f1  their harmonic mean
      purity        summary[6] / kept annotated points (summary[0] - summary[2]);  completeness  summary[7] / summary[0]
      ari           the adjusted Rand index over the annotated points, from c = summary[8], a = summary[9], b = summary[10], n = summary[0],
                    T = C(n, 2): (c - a b / T) / ((a + b) / 2 - a b / T), the dropped points as one class
    Any score whose denominator is zero is NaN.  tau must lie in [0.5, 1)."""
    tau = float(tau)
    if not 0.5 <= tau < 1.0:
        raise ValueError(f"tau = {tau} must lie in [0.5, 1)")
    s = [int(v) for v in cmp["summary"]]
    nan = float("nan")

    def div(a, b):
        return a / b if b != 0 else nan

    matched = int(np.count_nonzero(np.asarray(cmp["seg_best_iou"]) > tau))
    precision, recall = div(matched, s[5]), div(matched, s[3])
    f1 = div(2.0 * precision * recall, precision + recall) if precision == precision and recall == recall else nan
    n = s[0]
    T = n * (n - 1) // 2
    expected = div(float(s[9]) * float(s[10]), float(T))
    ari = div(float(s[8]) - expected, (float(s[9]) + float(s[10])) / 2.0 - expected) if expected == expected else nan
    return {"tau": tau, "matched": matched, "precision": precision, "recall": recall, "f1": f1, "purity": div(s[6], s[0] - s[2]),
            "completeness": div(s[7], s[0]), "ari": ari}


def default_params(method=2, **kw):
    p = VgsParams()
    L = _lib.lib()
    (L.vgs_params_default_svgs if method == 3 else L.vgs_params_default_vgs)(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def parse_task_file(path):
    """inputTaskTxtFile + the line indices of segmentationVGS/SVGS (point_clouds_IO.cpp:148-169, test:25-37,108-125)."""
    p = VgsParams()
    a = C.create_string_buffer(512)
    b = C.create_string_buffer(512)
    st = _lib.lib().vgs_parse_task_file(path.encode(), C.byref(p), a, b, 512)
    if st != _lib.VGS_OK:
        raise VgsError(st, f"cannot parse task file {path}")
    return p, a.value.decode(), b.value.decode()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class _Pinned:
    """Owner of one hipHostMalloc block (freed when the last numpy view of it goes away)."""

    def __init__(self, nbytes):
        self._L = _lib.lib()
        self.p = C.c_void_p()
        st = self._L.vgs_host_alloc(C.byref(self.p), max(int(nbytes), 1))
        if st != _lib.VGS_OK:
            raise VgsError(st, f"vgs_host_alloc({nbytes})")

    def __del__(self):
        try:
            if self.p.value:
                self._L.vgs_host_free(self.p)
                self.p = C.c_void_p()
        except Exception:
            pass


def pinned_empty(shape, dtype):
    """numpy array in pinned host memory (vgs_host_alloc): the staging buffers of stage_points / point_labels_async."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    blk = _Pinned(n)
    buf = (C.c_char * max(n, 1)).from_address(blk.p.value)
    buf._owner = blk   # the ctypes array keeps the block alive, the numpy array keeps the ctypes array alive
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


class Engine:
    def __init__(self, params: VgsParams):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.params = params
        st = self._L.vgs_create(C.byref(params), C.byref(self._h))
        if st != _lib.VGS_OK:
            raise VgsError(st, self._L.vgs_last_error_string(None).decode())
        self._keep = None
        self.n = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.vgs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        if st != _lib.VGS_OK:
            raise VgsError(st, self._L.vgs_last_error_string(self._h).decode())

    def set_params(self, params: VgsParams):
        self._ck(self._L.vgs_set_params(self._h, C.byref(params)))
        self.params = params

    # ---- input
    def set_points(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
            raise ValueError("xyz must be (N,3) or (N,4) float32")
        self._keep = xyz
        self.n = xyz.shape[0]
        self._ck(self._L.vgs_set_points(self._h, _ptr(xyz), xyz.shape[0], xyz.shape[1] * 4))

    def set_points_device(self, ptr, n, stride_bytes=12, keep=None):
        self._keep = keep
        self.n = int(n)
        self._ck(self._L.vgs_set_points_device(self._h, C.c_void_p(ptr), int(n), stride_bytes))

    # ---- stages
    def voxelize(self): self._ck(self._L.vgs_voxelize(self._h))
    def features(self): self._ck(self._L.vgs_features(self._h))
    def adjacency(self): self._ck(self._L.vgs_adjacency(self._h))
    def segment(self): self._ck(self._L.vgs_segment(self._h))
    def run(self): self._ck(self._L.vgs_run(self._h))

    # ---- SVGS
    def set_supervoxel_labels(self, labels, max_label):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape[0] != self.n:
            raise ValueError("one label per point required")
        self._ck(self._L.svgs_set_supervoxel_labels(self._h, _ptr(labels), int(max_label)))

    def supervoxels(self): self._ck(self._L.svgs_supervoxels(self._h))
    def svgs_segment(self): self._ck(self._L.svgs_segment(self._h))

    # ---- results
    def counts(self):
        c = np.zeros(_lib.N_COUNTS, dtype=np.int64)
        self._ck(self._L.vgs_get_counts(self._h, _ptr(c)))
        names = ["points", "finite", "voxels", "used", "adj", "clusters", "kept", "pairs", "depth", "isolated", "reattached",
                 "supervoxels", "handed_over", "class_a", "class_bc", "class_d"]  # 12..15: local-cut scheduling diagnostics
        return {k: int(c[i]) for i, k in enumerate(names)}

    def schedule_counters(self):
        c = np.zeros(13, dtype=np.int64)
        self._ck(self._L.vgs_get_schedule_counters_ex(self._h, _ptr(c), 13))
        names = ("lazy_gave_up", "list_overflow", "handed_over", "dense_sent_on", "handed_over_large", "outside_limits", "cross_put_off", "banded",
                 "extra_large", "pair_list_cut", "pair_list_entries", "voted_over", "pair_list_pool_full")
        return dict(zip(names, (int(x) for x in c)))

    def stage_times(self):
        t = np.zeros(_lib.T_COUNT, dtype=np.float64)
        self._ck(self._L.vgs_get_stage_times(self._h, _ptr(t)))
        names = ["voxelize", "features", "adjacency", "localcut", "merge", "labels", "total", "localcut_kernel", "supervoxel", "localcut_bulk"]
        return {k: float(t[i]) for i, k in enumerate(names)}

    def bbox(self):
        b = np.zeros(6, dtype=np.float64)
        self._ck(self._L.vgs_get_bbox(self._h, _ptr(b)))
        return b

    def voxel_table(self):
        c = self.counts()
        V, nf = c["voxels"], c["finite"]
        key = np.zeros((V, 3), dtype=np.uint32)
        start = np.zeros(V + 1, dtype=np.int32)
        pidx = np.zeros(nf, dtype=np.int32)
        self._ck(self._L.vgs_get_voxel_table(self._h, _ptr(key), _ptr(start), _ptr(pidx)))
        return dict(key=key, start=start, point_idx=pidx)

    def voxel_centers(self):
        V = self.counts()["voxels"]
        c = np.zeros((V, 3), dtype=np.float32)
        self._ck(self._L.vgs_get_voxel_centers(self._h, _ptr(c)))
        return c

    def point_voxel(self):
        out = np.zeros(self.n, dtype=np.int32)
        self._ck(self._L.vgs_get_point_voxel(self._h, _ptr(out)))
        return out

    def attributes(self):
        V = self.counts()["voxels"]
        cen = np.zeros((V, 3), dtype=np.float32)
        nrm = np.zeros((V, 3), dtype=np.float32)
        eig = np.zeros((V, 8), dtype=np.float32)
        used = np.zeros(V, dtype=np.uint8)
        self._ck(self._L.vgs_get_attributes(self._h, _ptr(cen), _ptr(nrm), _ptr(eig), _ptr(used)))
        return dict(centroid=cen, normal=nrm, eigen=eig, used=used)

    LISTS = {"adjacency": 0, "connect_cut": 1, "connect_cross": 2, "connect_final": 3}

    def lists(self, which, order="voxel_id"):
        """Ragged lists as (offsets, ids).  order="reference": the connect lists element for element as the reference holds them
        (merge-history order of the local cut, csrc/cutorder.hip); "voxel_id": members in adjacency-row order (the hot path's)."""
        V = self.counts()["voxels"]
        off = np.zeros(V + 1, dtype=np.int64)
        w, o = self.LISTS[which], self.ORDERS[order]
        self._ck(self._L.vgs_get_lists_ordered(self._h, w, o, _ptr(off), None))
        idx = np.zeros(max(int(off[-1]), 1), dtype=np.int32)
        self._ck(self._L.vgs_get_lists_ordered(self._h, w, o, _ptr(off), _ptr(idx)))
        return off, idx[:int(off[-1])]

    def adjacency_counts(self):
        """Neighbours inside graph_size per node, itself included (0 for unused voxels)."""
        out = np.zeros(self.counts()["voxels"], dtype=np.int32)
        self._ck(self._L.vgs_get_adjacency_counts(self._h, _ptr(out)))
        return out

    def local_weights(self, node_id):
        """(ids, W): the n x n affinity matrix of node_id's local graph over its stored adjacency row (W[a, b]: ids[a] first)."""
        n = C.c_int32(0)
        self._ck(self._L.vgs_get_local_weights(self._h, int(node_id), C.byref(n), None, None))
        ids = np.zeros(max(n.value, 1), dtype=np.int32)
        W = np.zeros((max(n.value, 1), max(n.value, 1)), dtype=np.float32)
        if n.value:
            self._ck(self._L.vgs_get_local_weights(self._h, int(node_id), C.byref(n), _ptr(ids), _ptr(W)))
        return ids[:n.value], W[:n.value, :n.value]

    def node_labels(self):
        V = self.counts()["voxels"]
        root = np.zeros(V, dtype=np.int32)
        kept = np.zeros(V, dtype=np.int32)
        self._ck(self._L.vgs_get_node_labels(self._h, _ptr(root), _ptr(kept)))
        return root, kept

    def point_labels(self):
        out = np.zeros(self.n, dtype=np.int32)
        self._ck(self._L.vgs_get_point_labels(self._h, _ptr(out)))
        return out

    def supervoxel_labels(self):
        """Per-point supervoxel labels of the last svgs_supervoxels / set_supervoxel_labels (0 = unassigned) and max_label."""
        out = np.zeros(self.n, dtype=np.int32)
        mx = C.c_int32(0)
        self._ck(self._L.svgs_get_supervoxel_labels(self._h, _ptr(out), C.byref(mx)))
        return out, int(mx.value)

    def point_labels_device_ptr(self):
        p = C.c_void_p()
        self._ck(self._L.vgs_get_point_labels_device(self._h, C.byref(p)))
        return p.value

    REFINE_COUNTS = ("working_nodes", "points_examined", "points_changed", "points_filled")

    def refine_labels(self, patch_radius=None, switch_ratio=0.25, fill=True):
        """Point-level label refinement at segment boundaries (include/vgs.h, vgs_refine_point_labels): every point of a node with a
        neighbour of another label takes the label of the node whose planar patch lies nearest, if that beats its own by switch_ratio;
        with fill the points of unused voxels and dropped clusters take the nearest labelled neighbour's.  patch_radius None: voxel_size
        (VGS) or seed_size (SVGS).  A new output next to point_labels(), read with refined_labels(); returns a dict of the counts
        (REFINE_COUNTS)."""
        rp = VgsRefineParams()
        self._ck(self._L.vgs_refine_params_default(self._h, C.byref(rp)))
        if patch_radius is not None:
            rp.patch_radius = float(patch_radius)
        rp.switch_ratio = float(switch_ratio)
        rp.fill = 1 if fill else 0
        cnt = np.zeros(4, dtype=np.int64)
        self._ck(self._L.vgs_refine_point_labels(self._h, C.byref(rp), _ptr(cnt)))
        return {name: int(v) for name, v in zip(self.REFINE_COUNTS, cnt)}

    def refined_labels(self):
        """The labels of the last refine_labels(), one int32 per input point; valid until the next run or the next refine."""
        out = np.zeros(self.n, dtype=np.int32)
        self._ck(self._L.vgs_get_refined_labels(self._h, _ptr(out)))
        return out

    def refined_labels_device_ptr(self):
        p = C.c_void_p()
        self._ck(self._L.vgs_get_refined_labels_device(self._h, C.byref(p)))
        return p.value

    ORDERS = {"voxel_id": 0, "reference": 1}

    def clusters(self, order="voxel_id"):
        """getClusterIdx as (offsets, point indices).  order="reference": nodes in recursionSearch's DFS order with the seed
        last, points per node ascending (voxel_segmentation.h:2032-2080, 981-999) -- the reference's own element order."""
        K = self.counts()["kept"]
        o = self.ORDERS[order]
        off = np.zeros(K + 1, dtype=np.int64)
        self._ck(self._L.vgs_get_clusters_ordered(self._h, o, _ptr(off), None))
        idx = np.zeros(max(int(off[-1]), 1), dtype=np.int32)
        self._ck(self._L.vgs_get_clusters_ordered(self._h, o, _ptr(off), _ptr(idx)))
        return off, idx[:int(off[-1])]

    def clusters_device(self):
        """getClusterIdx left in HBM: (device pointer of the offsets [kept + 1] int64, device pointer of the point indices int32)."""
        po, pi = C.c_void_p(), C.c_void_p()
        self._ck(self._L.vgs_get_clusters_device(self._h, C.byref(po), C.byref(pi)))
        return po.value, pi.value

    # per segment: (field, dtype, values per segment) of vgs_get_segment_descriptors, in its argument order
    DESCRIPTOR_FIELDS = (("n_points", np.int64, 1), ("n_nodes", np.int32, 1), ("bbox6", np.float32, 6), ("centroid3", np.float64, 3),
                         ("cov6", np.float64, 6), ("evals3", np.float64, 3), ("evecs9", np.float64, 9), ("eigen8", np.float32, 8))

    def segment_descriptors(self):
        """Geometric descriptors of the kept segments, row k = the points labelled k (include/vgs.h, vgs_get_segment_descriptors): a dict
        of numpy arrays n_points (K,), n_nodes (K,), bbox6 (K, 6), centroid3 (K, 3), cov6 (K, 6: xx xy xz yy yz zz), evals3 (K, 3,
        ascending), evecs9 (K, 9: [r*3+j] = component r of eigenvector j), eigen8 (K, 8).  Computed on the device, cached until the next run."""
        K = self.counts()["kept"]
        out = {name: np.zeros((K, w) if w > 1 else K, dtype=dt) for name, dt, w in self.DESCRIPTOR_FIELDS}
        self._ck(self._L.vgs_get_segment_descriptors(self._h, *(_ptr(out[name]) for name, _, _ in self.DESCRIPTOR_FIELDS)))
        return out

    def segment_descriptors_device(self):
        """The same table left in HBM: {field: device pointer}, valid until the next run."""
        ps = [C.c_void_p() for _ in self.DESCRIPTOR_FIELDS]
        self._ck(self._L.vgs_get_segment_descriptors_device(self._h, *(C.byref(p) for p in ps)))
        return {name: p.value for (name, _, _), p in zip(self.DESCRIPTOR_FIELDS, ps)}

    # per segment: (field, dtype, values per segment) of vgs_get_segment_boxes, in its argument order; BOX_FRAMES: its frame argument
    BOX_FIELDS = (("center3", np.float64, 3), ("half3", np.float64, 3), ("frame9", np.float64, 9), ("lo3", np.float64, 3),
                  ("hi3", np.float64, 3))
    BOX_FRAMES = {"principal": 0, "upright": 1}

    def _box_frame(self, frame):
        return int(self.BOX_FRAMES.get(frame, frame))   # (a name, or the C value: another one is the library's VGS_E_ARG)

    def segment_boxes(self, frame="principal"):
        """Oriented bounding boxes of the kept segments, row k = the points labelled k (include/vgs.h, vgs_get_segment_boxes): a dict of
        float64 arrays center3 (K, 3), half3 (K, 3), frame9 (K, 9: [r*3+j] = component r of axis j), lo3 (K, 3), hi3 (K, 3).
        frame="principal": the segment's PCA axes (evecs9 of segment_descriptors); "upright": z stays z, the horizontal axes are the PCA
        of the xy covariance.  Computed on the device, cached per frame until the next run."""
        K = self.counts()["kept"]
        out = {name: np.zeros((K, w), dtype=dt) for name, dt, w in self.BOX_FIELDS}
        self._ck(self._L.vgs_get_segment_boxes(self._h, self._box_frame(frame), *(_ptr(out[name]) for name, _, _ in self.BOX_FIELDS)))
        return out

    def segment_boxes_device(self, frame="principal"):
        """The same table left in HBM: {field: device pointer}, valid until the next run."""
        ps = [C.c_void_p() for _ in self.BOX_FIELDS]
        self._ck(self._L.vgs_get_segment_boxes_device(self._h, self._box_frame(frame), *(C.byref(p) for p in ps)))
        return {name: p.value for (name, _, _), p in zip(self.BOX_FIELDS, ps)}

    # per edge: (field, dtype, values per edge) of vgs_get_segment_graph, in its argument order
    GRAPH_FIELDS = (("seg_ab", np.int32, 2), ("n_pairs", np.int64, 1), ("n_finite", np.int64, 1), ("nodes_ab", np.int32, 2),
                    ("w_sum", np.float64, 1), ("w_min", np.float32, 1), ("w_max", np.float32, 1))

    def segment_graph(self):
        """Adjacency graph of the kept segments (include/vgs.h, vgs_get_segment_graph): a dict of numpy arrays seg_ab (E, 2: a < b),
        n_pairs (E,), n_finite (E,), nodes_ab (E, 2), w_sum (E,), w_min (E,), w_max (E,), edges in ascending (a, b) order.  The labels
        are those of point_labels / getClusterIdx.  Computed on the device, cached until the next run."""
        E = C.c_int64(0)
        self._ck(self._L.vgs_get_segment_graph(self._h, C.byref(E), *([None] * len(self.GRAPH_FIELDS))))
        out = {name: np.zeros((E.value, w) if w > 1 else E.value, dtype=dt) for name, dt, w in self.GRAPH_FIELDS}
        if E.value:
            self._ck(self._L.vgs_get_segment_graph(self._h, C.byref(E), *(_ptr(out[name]) for name, _, _ in self.GRAPH_FIELDS)))
        return out

    def segment_graph_device(self):
        """The same table left in HBM: (E, {field: device pointer}), valid until the next run."""
        E = C.c_int64(0)
        ps = [C.c_void_p() for _ in self.GRAPH_FIELDS]
        self._ck(self._L.vgs_get_segment_graph_device(self._h, C.byref(E), *(C.byref(p) for p in ps)))
        return E.value, {name: p.value for (name, _, _), p in zip(self.GRAPH_FIELDS, ps)}

    # per (segment, channel): (field, dtype) of vgs_segment_field_stats, in its argument order
    FIELD_STAT_FIELDS = (("n_valid", np.int64), ("anchor", np.float64), ("mean", np.float64), ("var", np.float64), ("vmin", np.float32),
                         ("vmax", np.float32))
    # per segment: (field, dtype, values per segment; 0 = n_classes) of vgs_segment_class_histogram, in its argument order
    CLASS_HIST_FIELDS = (("hist", np.int64, 0), ("n_outside", np.int64, 1), ("majority", np.int32, 1), ("majority_count", np.int64, 1))

    @staticmethod
    def _is_torch(a):
        return type(a).__module__.split(".")[0] == "torch"

    @staticmethod
    def _device_input(t, dtype_name, what, device):
        """A torch tensor on the context's device, complete before the library reads it on its own stream."""
        import torch
        if t.dtype != getattr(torch, dtype_name):
            raise ValueError(f"{what} must be {dtype_name}")
        if t.device.type != "cuda" or (t.device.index or 0) != int(device):
            raise ValueError(f"{what} must be a numpy array or a torch tensor on the context's device")
        torch.cuda.synchronize(t.device)

    @staticmethod
    def _field_input(field, device):
        """(array kept alive, pointer, n, channels, stride_bytes, on the device?) of a per-point attribute: float32 of shape (N,) or (N, C),
        C-contiguous or with a row stride (a multiple of 4 bytes; the channels of a row adjacent); a numpy array, or a torch tensor on the
        context's device, which is read in place."""
        if Engine._is_torch(field):
            Engine._device_input(field, "float32", "field", device)
            if field.dim() == 1:
                field = field.unsqueeze(1)
            if field.dim() != 2 or (field.shape[1] > 1 and field.stride(1) != 1) or (field.shape[0] > 1 and field.stride(0) < field.shape[1]):
                raise ValueError("field must be (N,) or (N, C) with adjacent channels and a row stride of at least C")
            n, ch = int(field.shape[0]), int(field.shape[1])
            return field, C.c_void_p(field.data_ptr()), n, ch, (int(field.stride(0)) * 4 if n > 1 else ch * 4), True
        field = np.asarray(field)
        if field.dtype != np.float32:
            raise ValueError("field must be float32")
        if field.ndim == 1:
            field = field[:, None]
        if field.ndim != 2:
            raise ValueError("field must be (N,) or (N, C)")
        n, ch = field.shape
        if (ch > 1 and field.strides[1] != 4) or (n > 1 and (field.strides[0] < 4 * ch or field.strides[0] % 4)):
            field = np.ascontiguousarray(field)   # (negative, interleaved or odd strides: the library takes rows of adjacent channels, 4-byte steps)
        return field, _ptr(field), n, ch, (int(field.strides[0]) if n > 1 else ch * 4), False

    @staticmethod
    def _classes_input(classes, device):
        """(array kept alive, pointer, n, on the device?) of a per-point class: int32 of shape (N,), numpy or a torch tensor on the device"""
        if Engine._is_torch(classes):
            Engine._device_input(classes, "int32", "classes", device)
            if classes.dim() != 1 or (classes.shape[0] > 1 and classes.stride(0) != 1):
                raise ValueError("classes must be a contiguous (N,) tensor")
            return classes, C.c_void_p(classes.data_ptr()), int(classes.shape[0]), True
        classes = np.asarray(classes)
        if classes.dtype != np.int32 or classes.ndim != 1:
            raise ValueError("classes must be int32 of shape (N,)")
        classes = np.ascontiguousarray(classes)
        return classes, _ptr(classes), classes.shape[0], False

    def segment_field_stats(self, field):
        """Per-segment statistics of a per-point attribute, row k = the points labelled k (include/vgs.h, vgs_segment_field_stats): a dict
        of arrays n_valid (int64), anchor, mean, var (float64), vmin, vmax (float32), each (K, C).  `field`: float32 of shape (N,) or (N, C)
        in input order, C-contiguous or with a row stride (a multiple of 4 bytes; the channels of a row adjacent); a numpy array, or a torch
        tensor on the context's device, which is read in place.  NaN and +-inf are skipped.  Computed on the device on every call,
        bit-identical from call to call."""
        K = self.counts()["kept"]
        field, ptr, n, ch, stride, dev = self._field_input(field, self.params.device)
        fn = self._L.vgs_segment_field_stats_device if dev else self._L.vgs_segment_field_stats
        out = {name: np.zeros((K, max(ch, 0)), dtype=dt) for name, dt in self.FIELD_STAT_FIELDS}
        self._ck(fn(self._h, ptr, n, ch, stride, *(_ptr(out[name]) for name, _ in self.FIELD_STAT_FIELDS)))
        return out

    def segment_class_histogram(self, classes, n_classes):
        """Per-segment histogram of a per-point class, row k = the points labelled k (include/vgs.h, vgs_segment_class_histogram): a dict of
        hist (K, n_classes) int64, n_outside (K,) int64 -- points whose class is negative or >= n_classes --, majority (K,) int32 -- the
        lowest class with the largest count, -1 without one -- and majority_count (K,) int64.  `classes`: int32 of shape (N,) in input
        order, a numpy array or a torch tensor on the context's device."""
        K = self.counts()["kept"]
        nc = int(n_classes)
        classes, ptr, n, dev = self._classes_input(classes, self.params.device)
        fn = self._L.vgs_segment_class_histogram_device if dev else self._L.vgs_segment_class_histogram
        out = {name: np.zeros((K, max(nc, 0)) if w == 0 else K, dtype=dt) for name, dt, w in self.CLASS_HIST_FIELDS}
        self._ck(fn(self._h, ptr, n, nc, *(_ptr(out[name]) for name, _, _ in self.CLASS_HIST_FIELDS)))
        return out

    # (field, dtype, table) of vgs_get_label_comparison, in its argument order; the tables have n_cells, G and K rows
    COMPARE_FIELDS = (("cell_seg", np.int32, "cells"), ("cell_ref", np.int32, "cells"), ("cell_n", np.int64, "cells"),
                      ("ref_id", np.int32, "refs"), ("ref_points", np.int64, "refs"), ("ref_dropped", np.int64, "refs"),
                      ("ref_best_seg", np.int32, "refs"), ("ref_best_n", np.int64, "refs"), ("ref_best_iou", np.float64, "refs"),
                      ("seg_annotated", np.int64, "segs"), ("seg_refs", np.int32, "segs"), ("seg_best_ref", np.int32, "segs"),
                      ("seg_best_n", np.int64, "segs"), ("seg_best_iou", np.float64, "segs"))

    def _labels_input(self, labels, K):
        """(array kept alive, pointer, n, on the device?, K) of a caller's per-point labelling: _classes_input's rules, K None = the
        engine's own kept count"""
        labels, ptr, n, dev = self._classes_input(labels, self.params.device)
        return labels, ptr, n, dev, (self.counts()["kept"] if K is None else int(K))

    def describe_labels(self, labels, K=None):
        """Descriptors of ANY per-point labelling of the cloud (include/vgs.h, vgs_point_label_descriptors): the dict of
        segment_descriptors(), K rows, row k = the points with labels[i] == k that are in the octree (the finite ones), plus n_skipped, the
        labelled points that are not.  `labels`: int32 of shape (N,) in input order, a numpy array or a torch tensor on the context's
        device, which is read in place; negative = no segment, a label >= K is an error.  K None: counts()["kept"], the range of
        point_labels() and refined_labels().  A label no point carries gives n_points 0 and a bbox6 of (+inf x3, -inf x3).  Computed on
        the device on every call, nothing cached; handed point_labels() it returns segment_descriptors() byte for byte."""
        labels, ptr, n, dev, K = self._labels_input(labels, K)
        fn = self._L.vgs_point_label_descriptors_device if dev else self._L.vgs_point_label_descriptors
        out = {name: np.zeros((max(K, 0), w) if w > 1 else max(K, 0), dtype=dt) for name, dt, w in self.DESCRIPTOR_FIELDS}
        skipped = C.c_int64(0)
        self._ck(fn(self._h, ptr, n, K, C.byref(skipped), *(_ptr(out[name]) for name, _, _ in self.DESCRIPTOR_FIELDS)))
        out["n_skipped"] = int(skipped.value)
        return out

    def label_boxes(self, labels, frame="principal", K=None):
        """Oriented boxes of ANY per-point labelling of the cloud (include/vgs.h, vgs_point_label_boxes): the dict of segment_boxes(), K
        rows, in the frames that describe_labels()' rows of the same labelling give.  `labels`, K as describe_labels().  A label no point
        carries gives lo = hi = half = 0 and center = its (zero) centroid."""
        labels, ptr, n, dev, K = self._labels_input(labels, K)
        fn = self._L.vgs_point_label_boxes_device if dev else self._L.vgs_point_label_boxes
        out = {name: np.zeros((max(K, 0), w), dtype=dt) for name, dt, w in self.BOX_FIELDS}
        self._ck(fn(self._h, ptr, n, K, self._box_frame(frame), *(_ptr(out[name]) for name, _, _ in self.BOX_FIELDS)))
        return out

    def _label_table_inputs(self, labels, other, what, K):
        """_labels_input for label_field_stats / label_class_histogram: labels and the attribute array both numpy or both torch tensors on
        the device.  (The library takes one n for both: the callers hand it the length that is not the cloud's, if one is not, so that
        its own VGS_E_ARG names the number.)"""
        if self._is_torch(labels) != self._is_torch(other):
            raise ValueError(f"labels and {what} must both be numpy arrays or both be torch tensors on the context's device")
        return self._labels_input(labels, K)

    def label_field_stats(self, labels, field, K=None):
        """Field statistics of ANY per-point labelling of the cloud (include/vgs.h, vgs_point_label_field_stats): the dict of
        segment_field_stats() with K rows, row k = the points with labels[i] == k that are in the octree, plus n_skipped, the labelled
        points that are not.  `labels`, K as describe_labels(); `field` as segment_field_stats(); both numpy arrays or both torch tensors
        on the context's device, which are read in place.  A label no point carries gives n_valid 0, anchor 0 and NaN.  Computed on the
        device on every call, nothing cached, bit-identical from call to call; handed point_labels() it returns segment_field_stats(field)
        byte for byte."""
        labels, lptr, ln, dev, K = self._label_table_inputs(labels, field, "field", K)
        field, ptr, n, ch, stride, _ = self._field_input(field, self.params.device)
        fn = self._L.vgs_point_label_field_stats_device if dev else self._L.vgs_point_label_field_stats
        out = {name: np.zeros((max(K, 0), max(ch, 0)), dtype=dt) for name, dt in self.FIELD_STAT_FIELDS}
        skipped = C.c_int64(0)
        self._ck(fn(self._h, lptr, K, ptr, ln if ln != self.n else n, ch, stride, C.byref(skipped),
                    *(_ptr(out[name]) for name, _ in self.FIELD_STAT_FIELDS)))
        out["n_skipped"] = int(skipped.value)
        return out

    def label_class_histogram(self, labels, classes, n_classes, K=None):
        """Class histogram of ANY per-point labelling of the cloud (include/vgs.h, vgs_point_label_class_histogram): the dict of
        segment_class_histogram() with K rows over the octree points of every label, plus n_skipped.  `labels`, K as describe_labels();
        `classes` as segment_class_histogram(); both numpy arrays or both torch tensors on the context's device.  hist.sum(1) + n_outside
        equals describe_labels(labels, K)["n_points"]; handed point_labels() it returns segment_class_histogram() byte for byte."""
        nc = int(n_classes)
        labels, lptr, ln, dev, K = self._label_table_inputs(labels, classes, "classes", K)
        classes, ptr, n, _ = self._classes_input(classes, self.params.device)
        fn = self._L.vgs_point_label_class_histogram_device if dev else self._L.vgs_point_label_class_histogram
        out = {name: np.zeros((max(K, 0), max(nc, 0)) if w == 0 else max(K, 0), dtype=dt) for name, dt, w in self.CLASS_HIST_FIELDS}
        skipped = C.c_int64(0)
        self._ck(fn(self._h, lptr, K, ptr, ln if ln != self.n else n, nc, C.byref(skipped),
                    *(_ptr(out[name]) for name, _, _ in self.CLASS_HIST_FIELDS)))
        out["n_skipped"] = int(skipped.value)
        return out

    # (field, dtype, table) of vgs_get_point_label_components, in its argument order; the tables have N, C, K + 1 and K rows
    COMPONENT_FIELDS = (("part_of_point", np.int32, "points"), ("part_label", np.int32, "parts"), ("part_points", np.int64, "parts"),
                        ("part_nodes", np.int32, "parts"), ("part_first_node", np.int32, "parts"), ("label_first", np.int64, "first"),
                        ("label_largest", np.int32, "labels"))

    def label_components(self, labels, K=None):
        """Connected parts of ANY per-point labelling of the cloud (include/vgs.h, vgs_point_label_components): a dict of numpy arrays --
        part_of_point (N, int32; -1 for a point without label or without node), part_label, part_points (int64), part_nodes,
        part_first_node (C rows, parts in ascending (label, smallest node id)), label_first (K + 1, int64: the parts of label k are
        label_first[k] .. label_first[k + 1] - 1), label_largest (K; -1 for a label no point carries) -- plus n_parts = C and n_skipped,
        the labelled points outside the octree.  Two vertices (label, node) are joined when either node's row of lists(0) holds the other.
        `labels`: int32 of shape (N,) in input order, a numpy array or a torch tensor on the context's device, which is read in place;
        negative = no label, a label >= K is an error.  K None: max(label) + 1 (0 for an empty or all-negative labelling) -- the range
        of a class field or of instance ids is the caller's, not the engine's kept count.  Computed on the device; integers only,
        bit-identical from call to call.  part_of_point is itself a labelling with K = n_parts: every label_* table applies to it."""
        if K is None:
            if self._is_torch(labels):
                K = max(int(labels.max().item()) + 1, 0) if labels.numel() > 0 else 0
            else:
                a = np.asarray(labels)
                K = max(int(a.max()) + 1, 0) if a.size > 0 else 0
        labels, ptr, n, dev, K = self._labels_input(labels, K)
        fn = self._L.vgs_point_label_components_device if dev else self._L.vgs_point_label_components
        n_parts, skipped = C.c_int64(0), C.c_int64(0)
        self._ck(fn(self._h, ptr, n, K, C.byref(n_parts), C.byref(skipped)))
        rows = {"points": self.n, "parts": n_parts.value, "first": max(K, 0) + 1, "labels": max(K, 0)}
        out = {name: np.zeros(rows[tab], dtype=dt) for name, dt, tab in self.COMPONENT_FIELDS}
        self._ck(self._L.vgs_get_point_label_components(self._h, *(_ptr(out[name]) for name, _, _ in self.COMPONENT_FIELDS)))
        out["n_parts"] = int(n_parts.value)
        out["n_skipped"] = int(skipped.value)
        return out

    def label_components_device(self):
        """The tables of the last label_components left in HBM: {field: device pointer, None for a table without rows}, valid until the
        next label_components or the next run."""
        ps = [C.c_void_p() for _ in self.COMPONENT_FIELDS]
        self._ck(self._L.vgs_get_point_label_components_device(self._h, *(C.byref(p) for p in ps)))
        return {name: p.value for (name, _, _), p in zip(self.COMPONENT_FIELDS, ps)}

    # per edge: (field, dtype, values per edge) of vgs_get_point_label_graph, in its argument order
    LABEL_GRAPH_FIELDS = (("seg_ab", np.int32, 2), ("n_shared", np.int64, 1), ("n_pairs", np.int64, 1), ("n_finite", np.int64, 1),
                          ("nodes_ab", np.int32, 2), ("w_sum", np.float64, 1), ("w_min", np.float32, 1), ("w_max", np.float32, 1))

    def label_graph(self, labels, K=None):
        """Adjacency graph of ANY per-point labelling of the cloud (include/vgs.h, vgs_point_label_graph): a dict of numpy arrays, one row
        per edge {a < b} in ascending (a, b) -- seg_ab (E, 2), n_shared (nodes that carry both labels), n_pairs (contacts: pairs of
        adjacent nodes, one carrying a and the other b, each counted once), n_finite, nodes_ab (E, 2: the (label, node) vertices of a
        and of b that are in a contact), w_sum, w_min, w_max (the local cut's weight over the contacts between two used nodes) -- plus
        n_edges = E and n_skipped, the labelled points outside the octree.  Adjacency is that of label_components(): either node's row
        of lists(0) holds the other.  `labels`, K as label_components() (K None: max(label) + 1).  Computed on the device, bit-identical
        from call to call; handed point_labels() with K = counts()["kept"] it returns segment_graph() with n_shared = 0."""
        if K is None:
            if self._is_torch(labels):
                K = max(int(labels.max().item()) + 1, 0) if labels.numel() > 0 else 0
            else:
                a = np.asarray(labels)
                K = max(int(a.max()) + 1, 0) if a.size > 0 else 0
        labels, ptr, n, dev, K = self._labels_input(labels, K)
        fn = self._L.vgs_point_label_graph_device if dev else self._L.vgs_point_label_graph
        E, skipped = C.c_int64(0), C.c_int64(0)
        self._ck(fn(self._h, ptr, n, K, C.byref(E), C.byref(skipped)))
        out = {name: np.zeros((E.value, w) if w > 1 else E.value, dtype=dt) for name, dt, w in self.LABEL_GRAPH_FIELDS}
        self._ck(self._L.vgs_get_point_label_graph(self._h, *(_ptr(out[name]) for name, _, _ in self.LABEL_GRAPH_FIELDS)))
        out["n_edges"] = int(E.value)
        out["n_skipped"] = int(skipped.value)
        return out

    def label_graph_device(self):
        """The table of the last label_graph left in HBM: (E, {field: device pointer, None for E = 0}), valid until the next label_graph
        or the next run."""
        E = C.c_int64(0)
        ps = [C.c_void_p() for _ in self.LABEL_GRAPH_FIELDS]
        self._ck(self._L.vgs_get_point_label_graph_device(self._h, C.byref(E), *(C.byref(p) for p in ps)))
        return E.value, {name: p.value for (name, _, _), p in zip(self.LABEL_GRAPH_FIELDS, ps)}

    # the eight counts of vgs_absorb_point_label_parts, in their order
    ABSORB_COUNTS = ("rounds", "parts_absorbed", "points_relabelled", "candidates_left", "candidate_points_left", "points_dropped",
                     "n_parts", "n_skipped")

    def absorb_label_parts(self, labels, min_points=0, island_points=0, max_rounds=8, drop=False, K=None):
        """Absorb the stranded and the small connected parts of ANY per-point labelling into the neighbour they touch most (include/vgs.h,
        vgs_absorb_point_label_parts, which states the rule): a part of label_components(labels) with fewer than min_points points, or
        fewer than island_points when it is not the largest part of its label, takes the label of the stable part it shares the most
        boundary with (n_shared + n_pairs of label_graph over the parts; then the bigger part, then the lower part id); repeated for at
        most max_rounds rounds, since a small part's only neighbour can itself be small.  drop: what is still a candidate at the end
        gets -1.  `labels`, K as label_components() (K None: max(label) + 1); the input is never written.  Returns a dict: labels (numpy
        int32, N, input order) and the eight counts by name (ABSORB_COUNTS).  Integers only, bit-identical from call to call.  The call
        overwrites the results of label_components() and label_graph(): their *_device() getters raise until their next compute call."""
        if K is None:
            if self._is_torch(labels):
                K = max(int(labels.max().item()) + 1, 0) if labels.numel() > 0 else 0
            else:
                a = np.asarray(labels)
                K = max(int(a.max()) + 1, 0) if a.size > 0 else 0
        labels, ptr, n, dev, K = self._labels_input(labels, K)
        fn = self._L.vgs_absorb_point_label_parts_device if dev else self._L.vgs_absorb_point_label_parts
        ap = _lib.AbsorbParams(int(min_points), int(island_points), int(max_rounds), 1 if drop else 0)
        counts = np.zeros(8, dtype=np.int64)
        self._ck(fn(self._h, ptr, n, K, C.byref(ap), _ptr(counts)))
        out = {"labels": self.absorbed_labels()}
        out.update({name: int(v) for name, v in zip(self.ABSORB_COUNTS, counts)})
        return out

    def absorbed_labels(self):
        """The labelling of the last absorb_label_parts (numpy int32, N, input order), valid until the next one or the next run."""
        out = np.zeros(self.n, dtype=np.int32)
        self._ck(self._L.vgs_get_absorbed_point_labels(self._h, _ptr(out)))
        return out

    def absorbed_labels_device_ptr(self):
        """The same labelling left in HBM: its device pointer (None for an empty cloud), valid until the next absorb_label_parts or the
        next run."""
        p = C.c_void_p()
        self._ck(self._L.vgs_get_absorbed_point_labels_device(self._h, C.byref(p)))
        return p.value

    def compare_labels(self, ref, labels=None, K=None):
        """Score the segmentation against a labelling of the same points (include/vgs.h, vgs_compare_labels): the sparse contingency table
        between point_labels() and `ref`, the reference table and the segment table, as a dict of numpy arrays -- cell_seg, cell_ref, cell_n
        (one row per distinct (label, id) pair, ascending, the -1 row first), ref_id, ref_points, ref_dropped, ref_best_seg, ref_best_n,
        ref_best_iou (one row per distinct id, ascending), seg_annotated, seg_refs, seg_best_ref, seg_best_n, seg_best_iou (K rows) -- plus
        summary (int64[12]).  `ref`: int32 of shape (N,) in input order, a numpy array or a torch tensor on the context's device, which is
        read in place; a negative id marks a point without annotation.  Computed on the device; integer counts and single fp64 quotients,
        bit-identical from call to call.  comparison_scores() turns the dict into precision, recall, F1, purity and the Rand index.
        `labels` (include/vgs.h, vgs_compare_point_labels): score this per-point labelling instead of point_labels() -- refined_labels(),
        say -- with K segment rows (None: counts()["kept"]); int32 of shape (N,), negative = dropped, a label >= K is an error; numpy or a
        torch tensor on the context's device, as `ref` is (both of one kind)."""
        n_cells, n_refs = C.c_int64(0), C.c_int64(0)
        summary = np.zeros(12, np.int64)
        if labels is None:
            K = self.counts()["kept"]
            ref, ptr, n, dev = self._classes_input(ref, self.params.device)
            fn = self._L.vgs_compare_labels_device if dev else self._L.vgs_compare_labels
            self._ck(fn(self._h, ptr, n, C.byref(n_cells), C.byref(n_refs), _ptr(summary)))
        else:
            if self._is_torch(ref) != self._is_torch(labels):
                raise ValueError("ref and labels must both be numpy arrays or both be torch tensors on the context's device")
            ref, ptr, n, dev = self._classes_input(ref, self.params.device)
            labels, lptr, ln, _, K = self._labels_input(labels, K)
            if ln != n:
                raise ValueError("ref and labels must have the same length")
            fn = self._L.vgs_compare_point_labels_device if dev else self._L.vgs_compare_point_labels
            self._ck(fn(self._h, lptr, K, ptr, n, C.byref(n_cells), C.byref(n_refs), _ptr(summary)))
        rows = {"cells": n_cells.value, "refs": n_refs.value, "segs": max(K, 0)}
        out = {name: np.zeros(rows[tab], dtype=dt) for name, dt, tab in self.COMPARE_FIELDS}
        self._ck(self._L.vgs_get_label_comparison(self._h, *(_ptr(out[name]) for name, _, _ in self.COMPARE_FIELDS)))
        out["summary"] = summary
        return out

    def label_comparison_from_cells(self, cell_seg, cell_ref, cell_n, n_unannotated=0, K=None):
        """The dict of compare_labels() from a list of contingency cells instead of points (include/vgs.h,
        vgs_label_comparison_from_cells): cell_seg, cell_ref (int32) and cell_n (int64) of equal length, in any order and with any number
        of entries for one (segment, id) pair -- the lists several ranks counted over their own points, one after another.  The cells are
        merged and the tables built on the device; integer adds only, so the order of the input does not matter.  summary[1] =
        n_unannotated.  K: the number of segment rows, the engine's own kept count by default.  The tables become the engine's last
        comparison (label_comparison_device())."""
        K = self.counts()["kept"] if K is None else int(K)
        seg = np.ascontiguousarray(np.asarray(cell_seg, dtype=np.int32).reshape(-1))
        ref = np.ascontiguousarray(np.asarray(cell_ref, dtype=np.int32).reshape(-1))
        cnt = np.ascontiguousarray(np.asarray(cell_n, dtype=np.int64).reshape(-1))
        if not (seg.shape == ref.shape == cnt.shape):
            raise ValueError("cell_seg, cell_ref and cell_n must have the same length")
        n_cells, n_refs = C.c_int64(0), C.c_int64(0)
        summary = np.zeros(12, np.int64)
        self._ck(self._L.vgs_label_comparison_from_cells(self._h, K, seg.shape[0], _ptr(seg), _ptr(ref), _ptr(cnt), int(n_unannotated),
                                                         C.byref(n_cells), C.byref(n_refs), _ptr(summary)))
        rows = {"cells": n_cells.value, "refs": n_refs.value, "segs": K}
        out = {name: np.zeros(rows[tab], dtype=dt) for name, dt, tab in self.COMPARE_FIELDS}
        self._ck(self._L.vgs_get_label_comparison(self._h, *(_ptr(out[name]) for name, _, _ in self.COMPARE_FIELDS)))
        out["summary"] = summary
        return out

    def label_comparison_device(self):
        """The tables of the last compare_labels left in HBM: {field: device pointer, None for a table without rows}, valid until the next
        compare or the next run."""
        ps = [C.c_void_p() for _ in self.COMPARE_FIELDS]
        self._ck(self._L.vgs_get_label_comparison_device(self._h, *(C.byref(p) for p in ps)))
        return {name: p.value for (name, _, _), p in zip(self.COMPARE_FIELDS, ps)}

    # ---- a sequence of clouds: uploads of the next cloud and downloads of the last labels overlap the stages
    def stage_points(self, xyz):
        """Start the copy of the NEXT cloud (ideally a pinned array, see pinned_empty) and return at once."""
        if xyz.dtype != np.float32 or not xyz.flags["C_CONTIGUOUS"] or xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
            raise ValueError("xyz must be a C-contiguous (N,3) or (N,4) float32 array")
        self._staged = xyz
        self._ck(self._L.vgs_stage_points(self._h, _ptr(xyz), xyz.shape[0], xyz.shape[1] * 4))

    def commit_points(self):
        self._ck(self._L.vgs_commit_points(self._h))
        self._keep, self._staged = self._staged, None
        self.n = self._keep.shape[0]

    def point_labels_async(self, out):
        if out.dtype != np.int32 or not out.flags["C_CONTIGUOUS"] or out.shape[0] < self.n:
            raise ValueError("out must be a C-contiguous int32 array with one entry per point")
        self._labels_out = out
        self._ck(self._L.vgs_get_point_labels_async(self._h, _ptr(out)))

    def wait_labels(self):
        self._ck(self._L.vgs_wait_point_labels(self._h))


class VoxelBasedSegmentation:
    """pcl::VoxelBasedSegmentation<PointXYZ> (voxel_segmentation.h:57-2305), same member names and call order."""

    def __init__(self, input_resolution, device=0):          # VS:84
        self._p = default_params(2, voxel_size=float(input_resolution), device=device)
        self._eng = Engine(self._p)
        self._cloud = None
        self._drawn = False
        self._adj = None

    def _push(self):
        self._eng.set_params(self._p)

    # inherited PCL surface used by the driver (test:52-56)
    def setInputCloud(self, cloud):
        self._cloud = np.ascontiguousarray(cloud, dtype=np.float32)

    def getCloudPointNum(self, cloud):                       # VS:94
        self._cloud = np.ascontiguousarray(cloud, dtype=np.float32)
        return int(self._cloud.shape[0])

    def addPointsFromInputCloud(self):                       # test:54
        if self._cloud is None:
            raise VgsError(_lib.VGS_E_STATE, "addPointsFromInputCloud before setInputCloud")
        self._eng.set_points(self._cloud)
        self._eng.voxelize()

    def setVoxelSize(self, input_resolution, points_num_min, voxels_num_min, voxels_adj_min):  # VS:124
        # stored only (VS:127): the octree keeps binning with the constructor's resolution (VS:84)
        self.voxel_resolution_ = float(input_resolution)
        self._p.points_min = int(points_num_min)
        self._p.voxels_min = int(voxels_num_min)
        self._p.adjacency_min = int(voxels_adj_min)
        self._push()

    def getBoundingBox(self):                                # test:56
        return tuple(self._eng.bbox())

    def setBoundingBox(self, *args):                         # VS:133 (the engine keeps the octree's own box)
        pass

    def setVoxelCenters(self):                               # VS:146
        if self._eng.counts()["points"] and self._eng.stage_times()["voxelize"] == 0.0:
            self._eng.voxelize()

    def getVoxelCenters(self):                               # VS:191
        return self._eng.voxel_centers()

    def getVoxelNum(self):                                   # VS:104
        return self._eng.counts()["voxels"]

    def calcualteVoxelCloudAttributes(self, cloud=None):     # VS:290 (sic)
        self._eng.features()

    def findAllVoxelAdjacency(self, graph_size):             # VS:223
        self._p.graph_size = float(graph_size)
        self._push()
        self._eng.adjacency()
        self._adj = None

    def getOneVoxelAdjacency(self, voxel_id):                # VS:268
        if self._adj is None:    # fetched once per findAllVoxelAdjacency, not once per call
            self._adj = self._eng.lists("adjacency")
        off, idx = self._adj
        return idx[off[voxel_id]:off[voxel_id + 1]].tolist()

    def segmentVoxelCloudWithGraphModel(self, cut_thred, sig_p, sig_n, sig_o, sig_e, sig_c, sig_w):  # VS:372
        q = self._p
        q.cut_thred, q.sig_p, q.sig_n, q.sig_o, q.sig_e, q.sig_c, q.sig_w = (float(v) for v in (
            cut_thred, sig_p, sig_n, sig_o, sig_e, sig_c, sig_w))
        self._push()
        self._eng.segment()

    def drawColorMapofPointsinClusters(self, output_cloud=None):  # VS:947 "This is obligatory!"
        self._drawn = True
        return self._eng.point_labels()

    def getClusterNum(self):                                 # VS:111
        return self._eng.counts()["clusters"]

    def getClusterIdx(self):                                 # VS:117
        if not self._drawn:
            return []   # clusters_point_idx_ is only filled by drawColorMapofPointsinClusters (VS:1006)
        off, idx = self._eng.clusters("reference")
        return [idx[off[k]:off[k + 1]].tolist() for k in range(len(off) - 1)]

    def getClusterDescriptors(self):
        """Extension (no VS line): descriptor i describes getClusterIdx()[i] -- both are in label order (Engine.segment_descriptors)."""
        if not self._drawn:
            return {name: np.zeros((0, w) if w > 1 else 0, dtype=dt) for name, dt, w in Engine.DESCRIPTOR_FIELDS}
        return self._eng.segment_descriptors()

    def getClusterBoxes(self, frame="principal"):
        """Extension (no VS line): box i bounds getClusterIdx()[i] -- both are in label order (Engine.segment_boxes)."""
        if not self._drawn:
            return {name: np.zeros((0, w), dtype=dt) for name, dt, w in Engine.BOX_FIELDS}
        return self._eng.segment_boxes(frame)

    def getClusterGraph(self):
        """Extension (no VS line): the adjacency graph of the kept clusters, labels = getClusterIdx() indices (Engine.segment_graph)."""
        if not self._drawn:
            return {name: np.zeros((0, w) if w > 1 else 0, dtype=dt) for name, dt, w in Engine.GRAPH_FIELDS}
        return self._eng.segment_graph()

    def getClusterFieldStats(self, field):
        """Extension (no VS line): row i reduces `field` over getClusterIdx()[i] -- both are in label order (Engine.segment_field_stats)."""
        if not self._drawn:
            ch = 1 if np.ndim(field) == 1 else int(np.shape(field)[1])
            return {name: np.zeros((0, ch), dtype=dt) for name, dt in Engine.FIELD_STAT_FIELDS}
        return self._eng.segment_field_stats(field)

    def getClusterClassHistogram(self, classes, n_classes):
        """Extension (no VS line): row i counts `classes` over getClusterIdx()[i] -- both are in label order (Engine.segment_class_histogram)."""
        if not self._drawn:
            return {name: np.zeros((0, int(n_classes)) if w == 0 else 0, dtype=dt) for name, dt, w in Engine.CLASS_HIST_FIELDS}
        return self._eng.segment_class_histogram(classes, n_classes)

    def compareClusterLabels(self, ref, labels=None):
        """Extension (no VS line): the clusters against a reference labelling; row i of the cluster table belongs to getClusterIdx()[i]
        (Engine.compare_labels).  `labels`: score this per-point labelling (refineClusterLabels()' result, say) instead of the clusters'
        own.  Empty tables and a zero summary before drawColorMapofPointsinClusters."""
        if not self._drawn:
            return dict({name: np.zeros(0, dtype=dt) for name, dt, _ in Engine.COMPARE_FIELDS}, summary=np.zeros(12, np.int64))
        return self._eng.compare_labels(ref, labels)

    def getLabelDescriptors(self, labels):
        """Extension (no VS line): the descriptors of a per-point labelling with the clusters' label range (refineClusterLabels()' result,
        say): row i describes the points labelled i, plus n_skipped (Engine.describe_labels).  Empty before
        drawColorMapofPointsinClusters."""
        if not self._drawn:
            return dict({name: np.zeros((0, w) if w > 1 else 0, dtype=dt) for name, dt, w in Engine.DESCRIPTOR_FIELDS}, n_skipped=0)
        return self._eng.describe_labels(labels)

    def getLabelBoxes(self, labels, frame="principal"):
        """Extension (no VS line): the oriented boxes of a per-point labelling with the clusters' label range (Engine.label_boxes).  Empty
        before drawColorMapofPointsinClusters."""
        if not self._drawn:
            return {name: np.zeros((0, w), dtype=dt) for name, dt, w in Engine.BOX_FIELDS}
        return self._eng.label_boxes(labels, frame)

    def getLabelComponents(self, labels):
        """Extension (no VS line): the connected parts of a per-point labelling with the clusters' label range (refineClusterLabels()'
        result, say) over the voxel adjacency: the dict of Engine.label_components with K = getClusterNum().  No part and every point -1
        before drawColorMapofPointsinClusters."""
        if not self._drawn:
            rows = {"points": self._eng.n, "parts": 0, "first": 1, "labels": 0}
            out = {name: np.zeros(rows[tab], dtype=dt) for name, dt, tab in Engine.COMPONENT_FIELDS}
            out["part_of_point"][:] = -1
            return dict(out, n_parts=0, n_skipped=0)
        return self._eng.label_components(labels, self._eng.counts()["kept"])

    def refineClusterLabels(self, patch_radius=None, switch_ratio=0.25, fill=True):
        """Extension (no VS line): one label per input point, refined at the cluster boundaries; label i names getClusterIdx()[i]
        (Engine.refine_labels / refined_labels).  Every point -1 before drawColorMapofPointsinClusters."""
        if not self._drawn:
            return np.full(self._eng.n, -1, dtype=np.int32)
        self._eng.refine_labels(patch_radius, switch_ratio, fill)
        return self._eng.refined_labels()

    @property
    def engine(self):
        return self._eng


class SuperVoxelBasedSegmentation:
    """pcl::SuperVoxelBasedSegmentation<PointXYZ> (supervoxel_segmentation.h:58-2308), same member names and call order."""

    def __init__(self, input_resolution, device=0):                                   # SS:85
        self._p = default_params(3, voxel_size=float(input_resolution), device=device)
        self._eng = Engine(self._p)
        self._cloud = None

    def setInputCloud(self, cloud):
        self._cloud = np.ascontiguousarray(cloud, dtype=np.float32)

    def getCloudPointNum(self, cloud):                                                # SS:101
        self._cloud = np.ascontiguousarray(cloud, dtype=np.float32)
        return int(self._cloud.shape[0])

    def addPointsFromInputCloud(self):                                                # test:142 (own octree: bookkeeping only)
        self._eng.set_points(self._cloud)

    def setVoxelSize(self, input_resolution, points_num_min):                         # SS:143
        self._p.voxel_size = float(input_resolution)
        self._p.points_min = int(points_num_min)
        self._eng.set_params(self._p)

    def setSupervoxelSize(self, input_resolution, voxels_num_min, points_num_min, adjacency_num_min):  # SS:150
        self._p.seed_size = float(input_resolution)
        self._p.voxels_min = int(voxels_num_min)
        self._p.adjacency_min = int(adjacency_num_min)
        self._eng.set_params(self._p)

    def setGraphSize(self, small_resolution, large_resolution):                       # SS:159 (the small radius feeds nothing, SS:1438-1475)
        self._p.graph_size = float(large_resolution)
        self._eng.set_params(self._p)

    def setBoundingBox(self, *args):                                                  # SS:166
        pass

    def setSupervoxelCentersCentroids(self):                                          # SS:178 (own-octree bookkeeping)
        pass

    def setSupervoxelLabels(self, labels, max_label):
        """What pcl::SupervoxelClustering::getLabeledCloud / getMaxLabel return (SS:283-284), supplied by the caller."""
        self._eng.set_supervoxel_labels(labels, max_label)

    def getVoxelNum(self):                                                            # SS:111
        return self._eng.counts()["voxels"]

    def getSuperVoxelNum(self):                                                       # SS:118
        return self._eng.counts()["supervoxels"]

    def segmentSupervoxelCloudWithGraphModel(self, sig_a, sig_b, sig_l, cut_thred, sig_p, sig_n, sig_o, sig_e, sig_c, sig_w):  # SS:362
        q = self._p
        q.color_impt, q.spatial_impt, q.normal_impt = float(sig_a), float(sig_b), float(sig_l)
        q.cut_thred, q.sig_p, q.sig_n, q.sig_o, q.sig_e, q.sig_c, q.sig_w = (float(v) for v in (
            cut_thred, sig_p, sig_n, sig_o, sig_e, sig_c, sig_w))
        self._eng.set_params(q)
        self._eng.run()   # createSupervoxels unless the caller's labelling of THIS cloud is in place, then the graph stages

    def drawColorMapofPointsinClusters(self, output_cloud=None):                      # SS:613
        return self._eng.point_labels()

    def getClusterNum(self):                                                          # SS:124
        return self._eng.counts()["clusters"]

    def getClusterIdx(self):                                                          # SS:130
        off, idx = self._eng.clusters("reference")
        return [idx[off[k]:off[k + 1]].tolist() for k in range(len(off) - 1)]

    def getClusterDescriptors(self):
        """Extension (no SS line): descriptor i describes getClusterIdx()[i] -- both are in label order (Engine.segment_descriptors)."""
        return self._eng.segment_descriptors()

    def getClusterBoxes(self, frame="principal"):
        """Extension (no SS line): box i bounds getClusterIdx()[i] -- both are in label order (Engine.segment_boxes)."""
        return self._eng.segment_boxes(frame)

    def getClusterGraph(self):
        """Extension (no SS line): the adjacency graph of the kept clusters, labels = getClusterIdx() indices (Engine.segment_graph)."""
        return self._eng.segment_graph()

    def getClusterFieldStats(self, field):
        """Extension (no SS line): row i reduces `field` over getClusterIdx()[i] -- both are in label order (Engine.segment_field_stats)."""
        return self._eng.segment_field_stats(field)

    def getClusterClassHistogram(self, classes, n_classes):
        """Extension (no SS line): row i counts `classes` over getClusterIdx()[i] -- both are in label order (Engine.segment_class_histogram)."""
        return self._eng.segment_class_histogram(classes, n_classes)

    def compareClusterLabels(self, ref, labels=None):
        """Extension (no SS line): the clusters against a reference labelling; row i of the cluster table belongs to getClusterIdx()[i]
        (Engine.compare_labels).  `labels`: score this per-point labelling (refineClusterLabels()' result, say) instead of the clusters'
        own."""
        return self._eng.compare_labels(ref, labels)

    def getLabelDescriptors(self, labels):
        """Extension (no SS line): the descriptors of a per-point labelling with the clusters' label range (refineClusterLabels()' result,
        say): row i describes the points labelled i, plus n_skipped (Engine.describe_labels)."""
        return self._eng.describe_labels(labels)

    def getLabelBoxes(self, labels, frame="principal"):
        """Extension (no SS line): the oriented boxes of a per-point labelling with the clusters' label range (Engine.label_boxes)."""
        return self._eng.label_boxes(labels, frame)

    def getLabelComponents(self, labels):
        """Extension (no SS line): the connected parts of a per-point labelling with the clusters' label range over the supervoxel
        adjacency: the dict of Engine.label_components with K = getClusterNum()."""
        return self._eng.label_components(labels, self._eng.counts()["kept"])

    def refineClusterLabels(self, patch_radius=None, switch_ratio=0.25, fill=True):
        """Extension (no SS line): one label per input point, refined at the cluster boundaries; label i names getClusterIdx()[i]
        (Engine.refine_labels / refined_labels)."""
        self._eng.refine_labels(patch_radius, switch_ratio, fill)
        return self._eng.refined_labels()

    @property
    def engine(self):
        return self._eng


def segmentation_vgs(cloud, params: VgsParams):
    """segmentationVGS (test:9-86) without file IO and viewer: returns (point labels, Engine)."""
    eng = Engine(params)
    eng.set_points(cloud)
    eng.run()
    return eng.point_labels(), eng
