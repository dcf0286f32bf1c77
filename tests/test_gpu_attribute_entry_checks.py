"""The order in which the 16 entry points of the attribute tables (field statistics, class histograms; csrc/segfield.hip,
csrc/pointfield.hip) check their arguments, through raw ctypes so that no Python-side validation answers first.  Four families -- the node
labelling and a caller's per-point labelling, each of one context and of a tile context -- two tables, host and _device variant.  Every
ladder starts from a call that breaks all of the family's rules at once and must fail with the FIRST rule's status and text; that argument
is repaired, the next rule must answer, and so on down to a valid call:
  node labels, one context     segment first, tile context refused, n, NULL input, n_channels, stride | n_classes
  node labels, tile context    segment first, not a tile context, K range, n_own, NULL input, n_channels, stride | n_classes, 2^27 limit
  point labels, one context    segment first, tile context refused, n, labels NULL, input NULL, K range, n_channels, stride, 2^27 limit |
                               n_classes, 2^27 limit
  point labels, tile context   segment first, not a tile context, K range, n_own, labels NULL, input NULL, n_channels, stride, 2^27 limit |
                               n_classes, 2^27 limit
"segment first" is asked of a fresh context, the tile rules of the other kind of context, the rest of one segmented context each.  The
own range against N, which stands between "input NULL" and n_channels / n_classes on the point family's tile ladder, is asked of a
context of its own whose range ends one point behind the cloud (vgs_set_own_point_range does not compare the range with the cloud).  One
rung is not asked: the 2^27 limit of the node histogram of one context (K is the context's own count: tests/test_gpu_segment_fields.py
builds the 131 073 segments it takes).  The early returns: without a label (K = 0), and on a tile context without an own point
(n_own = 0), the host variants return VGS_OK with n_records and n_skipped zero; a NULL context, and a NULL n_records where the node
family requires it, are VGS_E_ARG.  (n = 0 of one context is not asked: no segmented context has no point.)"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_segment_fields import _engine
from test_gpu_tiles_segdesc import _ranks

pytestmark = pytest.mark.gpu
OK, E_ARG, E_STATE, E_UNSUPPORTED = 0, 1, 2, 5
BIG = 1 << 27            # a K within either range whose table passes 2^27 entries at two columns
SEGMENT_FIRST = (E_STATE, "segment first")
TILE_REFUSED = (E_STATE, "holds only part")
TILE_ONLY = (E_STATE, "vgs_set_owned_region")
_cache = {}


def _ptr(x):
    """numpy array, torch tensor or None -> what a c_void_p argument takes"""
    if x is None:
        return None
    return x.ctypes.data_as(C.c_void_p) if isinstance(x, np.ndarray) else x.data_ptr()


class _Call:
    """One entry point: its argument names in the C order, the call that breaks every rule, and the rungs (status, word of the message,
    the repair) behind the state rules.  data: the valid field / cls / labels / n / K of the context the ladder runs on."""

    def __init__(self, family, table, device):
        self.family, self.table, self.device = family, table, device
        own, point = family.endswith("tile"), family.startswith("point")
        base = {("node_one", "field"): "vgs_segment_field_stats", ("node_one", "hist"): "vgs_segment_class_histogram",
                ("node_tile", "field"): "vgs_get_own_segment_field_moments", ("node_tile", "hist"): "vgs_get_own_segment_class_counts",
                ("point_one", "field"): "vgs_point_label_field_stats", ("point_one", "hist"): "vgs_point_label_class_histogram",
                ("point_tile", "field"): "vgs_own_point_label_field_moments", ("point_tile", "hist"): "vgs_own_point_label_class_counts"}
        self.name = base[family, table] + ("_device" if device else "")
        per = ["n_channels", "stride"] if table == "field" else ["n_classes"]
        tail = {"field": 6, "hist": 2 if own else 4}[table]                 # the output arrays: all NULL
        if not point:
            self.args = (["K"] if own else []) + ["in", "n"] + per + (["n_records", None] if own else []) + [None] * tail
        elif not own:
            self.args = ["labels", "K", "in", "n"] + per + ["n_skipped"] + [None] * tail
        else:
            self.args = ["K", "labels", "in", "n"] + per + ["n_records", "n_skipped", None] + [None] * tail
        self.own, self.point = own, point

    def broken(self, d):
        """every rule of the ladder broken at once"""
        return dict(K=(1 << 31) if self.point and not self.own else -1, labels=None, n=d["n"] - 1, n_channels=0, stride=6, n_classes=0)

    def rungs(self, d):
        n_word = "number of own points of the context" if self.own else "number of points of the cloud"
        k_range = (E_ARG, "out of range", dict(K=BIG))
        r = [k_range] if self.own else []
        r.append((E_ARG, n_word, dict(n=d["n"])))
        if self.point:
            r.append((E_ARG, "labels is NULL", dict(labels=d["labels"])))
        r.append((E_ARG, "the input array is NULL", {"in": d[self.table]}))
        if self.point and not self.own:
            r.append(k_range)
        if self.table == "field":
            r += [(E_ARG, "must be in 1 .. 64", dict(n_channels=2)), (E_ARG, "stride_bytes", dict(stride=8))]
        else:
            r.append((E_ARG, "must be in 1 .. 1024", dict(n_classes=2)))
        if self.point or (self.own and self.table == "hist"):
            r.append((E_UNSUPPORTED, "exceed the table's limit", dict(K=d["K"])))
        elif self.own:
            r[0] = (E_ARG, "out of range", dict(K=d["K"]))                  # the node field table has no limit: K straight to its value
        return r

    def __call__(self, L, h, values, n_records=None, n_skipped=None):
        """(status, message) of the call with the arguments `values`; n_records / n_skipped: ctypes words, made here when not given"""
        words = dict(n_records=n_records if n_records is not None else C.c_int64(7), n_skipped=n_skipped if n_skipped is not None else C.c_int64(7))
        argv = []
        for a in self.args:
            if a is None:
                argv.append(None)
            elif a in words:
                argv.append(C.byref(words[a]))
            elif a in ("in", "labels"):
                argv.append(_ptr(values.get(a)))
            else:
                argv.append(values[a])
        st = getattr(L, self.name)(h, *argv)
        return st, (L.vgs_last_error_string(h) or b"").decode() if st != OK and h is not None else ""


CALLS = [_Call(f, t, dev) for f in ("node_one", "node_tile", "point_one", "point_tile") for t in ("field", "hist") for dev in (False, True)]
IDS = [f"{c.family}-{c.table}-{'device' if c.device else 'host'}" for c in CALLS]


def _data(labels, kept, n, device):
    """the valid arguments of a context with n points (own points) and `kept` labels: two channels, two classes now and then out of range"""
    rng = np.random.default_rng(5)
    d = dict(n=n, K=kept, labels=np.ascontiguousarray(labels, dtype=np.int32), field=rng.integers(0, 100, (n, 2)).astype(np.float32),
             hist=rng.integers(-1, 3, n).astype(np.int32))
    if device:
        import torch
        d.update({k: torch.from_numpy(d[k]).to("cuda:0") for k in ("labels", "field", "hist")})
    return d


def _walk(L, h, call, d, state_rule=None):
    """-> [(got status, got message, wanted status, wanted word)]: the all-broken call (state_rule: only that, it must answer with the
    state rule given), then rung after rung, then the valid call"""
    values = call.broken(d)
    if state_rule is not None:
        return [call(L, h, values) + state_rule]
    out = []
    for status, word, repair in call.rungs(d) + [(OK, "", {})]:
        out.append(call(L, h, values) + (status, word))
        values.update(repair)
    return out


def _world(gpu):
    """One small cloud.  A fresh context, a segmented one and one without a kept segment; the same cloud as the only rank of a tile
    context, where everything that needs that context runs and is recorded: id of the call -> what _walk returns."""
    if "w" in _cache:
        return _cache["w"]
    L = gpu._lib.lib()
    xyz = gpu.scenes.town_scene(60_000)
    fresh = gpu.Engine(gpu.default_params(2))
    eng = _engine(gpu, xyz)
    kept = eng.counts()["kept"]
    labels = eng.point_labels()
    assert kept > 0 and labels.shape == (xyz.shape[0],)
    empty = _engine(gpu, xyz, voxels_min=10_000_000)
    assert empty.counts()["kept"] == 0
    plain = {dev: _data(labels, kept, xyz.shape[0], dev) for dev in (False, True)}

    def body(r, t, p):
        t.set_points(p)
        t.run()
        tl, tk = t.point_labels()
        assert tk > 0 and tl.shape == (p.shape[0],)
        h = t._ctx()
        rec = {}
        for call, cid in zip(CALLS, IDS):
            if call.own:
                rec[cid] = _walk(L, h, call, _data(tl, tk, p.shape[0], call.device))
            else:
                rec[cid] = _walk(L, h, call, plain[call.device], TILE_REFUSED)
        # K = 0 on the host variants: no record, nothing skipped
        d = _data(np.full(p.shape[0], -1, np.int32), 0, p.shape[0], False)
        for call, cid in zip(CALLS, IDS):
            if call.own and not call.device:
                nr, ns = C.c_int64(7), C.c_int64(7)
                st, _ = call(L, h, dict(K=0, labels=d["labels"], n=d["n"], n_channels=2, stride=8, n_classes=2, **{"in": d[call.table]}), nr, ns)
                rec[cid + "-K0"] = (st, nr.value, ns.value if call.point else 0)
        return rec
    out = _ranks(gpu, (1, 1), 1000.0, [xyz], body, params=gpu.default_params(2))
    assert not isinstance(out[0], Exception), out[0]
    _cache["w"] = dict(L=L, fresh=fresh, eng=eng, empty=empty, plain=plain, tile=out[0], n=xyz.shape[0])
    return _cache["w"]


def _assert_rungs(cid, rec):
    for i, (st, msg, want, word) in enumerate(rec):
        assert st == want and word in msg, (cid, i, st, msg, want, word)


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_check_order(gpu, call):
    w = _world(gpu)
    cid = IDS[CALLS.index(call)]
    L, d = w["L"], w["plain"][call.device]
    _assert_rungs(cid, _walk(L, w["fresh"]._h, call, d, SEGMENT_FIRST))
    if call.own:
        _assert_rungs(cid, _walk(L, w["eng"]._h, call, d, TILE_ONLY))      # a context with the whole cloud
        assert len(w["tile"][cid]) == len(call.rungs(d)) + 1
    else:
        _assert_rungs(cid, _walk(L, w["eng"]._h, call, d))
        assert len(w["tile"][cid]) == 1
    _assert_rungs(cid, w["tile"][cid])


def test_early_returns(gpu):
    w = _world(gpu)
    L, d = w["L"], w["plain"][False]
    unlabelled = np.full(w["n"], -1, np.int32)
    for call, cid in zip(CALLS, IDS):
        valid = dict(K=d["K"], labels=d["labels"], n=d["n"], n_channels=2, stride=8, n_classes=2, **{"in": d[call.table]})
        assert call(L, None, valid)[0] == E_ARG, cid                       # a NULL context
        if call.device:
            continue
        if call.own:
            assert w["tile"][cid + "-K0"] == (OK, 0, 0), cid
        elif call.point:                                                   # K = 0: validated, nothing skipped, nothing written
            ns = C.c_int64(7)
            assert call(L, w["eng"]._h, dict(valid, K=0, labels=unlabelled), n_skipped=ns) == (OK, "") and ns.value == 0, cid
        else:                                                              # no kept segment
            assert call(L, w["empty"]._h, valid) == (OK, ""), cid
    # the node family of a tile context requires n_records
    for name, args in (("vgs_get_own_segment_field_moments", (2, 8)), ("vgs_get_own_segment_class_counts", (2,))):
        for suffix in ("", "_device"):
            st = getattr(L, name + suffix)(w["eng"]._h, d["K"], _ptr(d["field"]), d["n"], *args, None, *([None] * (7 if len(args) == 2 else 3)))
            assert st == E_ARG, name + suffix


def _own_range_engine(gpu, xyz, first, n_own):
    """a segmented context with an owned region (everything) and the own point range given, as raw calls: vgs_set_own_point_range does
    not compare the range with the cloud"""
    eng = gpu.Engine(gpu.default_params(2))
    eng.set_points(xyz)
    lo, hi = np.array([-1e9, -1e9]), np.array([1e9, 1e9])
    eng._ck(eng._L.vgs_set_owned_region(eng._h, _ptr(lo), _ptr(hi)))
    eng._ck(eng._L.vgs_set_own_point_range(eng._h, first, n_own))
    eng.run()
    assert eng.counts()["kept"] > 0
    return eng


def _range_world(gpu):
    """two more tile contexts over the cloud: one whose own range ends one point behind the cloud, one without an own point"""
    if "r" not in _cache:
        xyz = gpu.scenes.town_scene(60_000)
        _cache["r"] = dict(n=xyz.shape[0], over=_own_range_engine(gpu, xyz, 0, xyz.shape[0] + 1), none=_own_range_engine(gpu, xyz, 0, 0))
    return _cache["r"]


@pytest.mark.parametrize("call", [c for c in CALLS if c.family == "point_tile"], ids=[i for c, i in zip(CALLS, IDS) if c.family == "point_tile"])
def test_own_range_against_the_cloud(gpu, call):
    """The own range against N stands between "input NULL" and the table's own rules: on a context whose range ends at N + 1 the ladder
    is walked down to the arrays, and the next answer names the range while n_channels, stride, n_classes and the limit are still broken.
    No call on this context passes its checks."""
    w = _range_world(gpu)
    L, h, n = gpu._lib.lib(), w["over"]._h, w["n"] + 1
    d = _data(np.full(n, -1, np.int32), w["over"].counts()["kept"], n, call.device)
    rungs = call.rungs(d)
    cut = 1 + max(i for i, r in enumerate(rungs) if "input array" in r[1])
    values = call.broken(d)
    for i, (status, word, repair) in enumerate(rungs[:cut]):
        st, msg = call(L, h, values)
        assert st == status and word in msg, (i, st, msg, status, word)
        values.update(repair)
    st, msg = call(L, h, values)
    assert st == E_ARG and f"the own point range ends at {n}, the cloud holds {n - 1} points" in msg, (st, msg)
    assert values["n_channels"] == 0 and values["n_classes"] == 0 and values["K"] == BIG


def test_no_own_point_returns_early(gpu):
    """n_own = 0: the host variants of both tile families return VGS_OK without a record (the node family before the device is touched)"""
    w = _range_world(gpu)
    L, eng = gpu._lib.lib(), w["none"]
    d = _data(np.full(1, -1, np.int32), eng.counts()["kept"], 1, False)
    for call, cid in zip(CALLS, IDS):
        if not call.own or call.device:
            continue
        nr, ns = C.c_int64(7), C.c_int64(7)
        st, msg = call(L, eng._h, dict(K=d["K"], labels=d["labels"], n=0, n_channels=2, stride=8, n_classes=2, **{"in": d[call.table]}), nr, ns)
        assert (st, msg) == (OK, "") and nr.value == 0, (cid, st, msg, nr.value)
        assert not call.point or ns.value == 0, (cid, ns.value)
