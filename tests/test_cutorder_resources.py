"""Resources of the reference-order replay (csrc/cutorder.hip), read from the compiler (hipcc cross-compiles gfx950 without a GPU).  Both
kernels index LDS arrays of CO_MAXK entries by the position inside a connect set: k_co_eval one uint16 array and a count, k_co_merge five
uint16 arrays and one of floats.  Neither may use scratch or spill, and the LDS the compiler allots must be what the source declares for
the cap -- a sixth array, or a cap the 64 KB of static LDS cannot hold, shows here before it shows on a device."""
import os
import re

import pytest

from test_kernel_resources import CSRC, HIPCC, _usage


def _cap():
    with open(os.path.join(CSRC, "cutorder_arith.h")) as f:
        return int(re.search(r"#define CO_MAXK (\d+)", f.read()).group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_replay_kernels_fit_their_declared_lds_without_scratch(tmp_path):
    cap = _cap()
    assert 4224 <= cap <= 65535      # at least the largest ball the local cut takes whole; indices are uint16 and 0xffff ends a list
    k = _usage("cutorder.hip", tmp_path)
    ev = [v for n, v in k.items() if n.startswith("_Z9k_co_eval")]
    mg = [v for n, v in k.items() if n.startswith("_Z10k_co_merge")]
    assert len(ev) == 1 and len(mg) == 1, sorted(k)
    for u in ev + mg:
        assert u["ScratchSize"] == 0, u
        assert u["VGPRs Spill"] == 0, u
    assert 2 * cap <= ev[0]["LDS Size"] <= 2 * cap + 16, ev[0]              # pos[] and s_k
    assert mg[0]["LDS Size"] == (5 * 2 + 4) * cap, mg[0]                   # pos, par, tail, nxt, ssz; thr
    assert mg[0]["LDS Size"] <= 65536, mg[0]
