"""CPU: the case list of tests/test_gpu_stem_edges.py (util.STEM_EDGE_CASES) still meets every launch edge of csrc/stem_gen.hip it was
chosen for. The geometry is recomputed from (F, H, W) alone (util.stem_case_props); the three constants it rests on are restated in
util.py with the source lines they come from: STEM_TILE = 256 (stem_fwd_gen_kernel: `m0 = blk * 256`), STEM_FWD_BLOCKS = 512
(launch_stem_fwd_gen: `grid = ntiles < 512 ? ntiles : 512`), STEM_WG_BLOCKS = 512 (csrc/stem_dev.h: `#define R3M_STEM_WG_BLOCKS 512`;
launch_stem_wgrad_gen: `nb`)."""
import ctypes as C
import os
import re

import pytest

from util import STEM_CONDITIONS, STEM_EDGE_CASES, STEM_FWD_BLOCKS, STEM_TILE, STEM_WG_BLOCKS, stem_case_props

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "r3m_amd", "csrc")


def test_the_restated_constants_are_the_sources():
    gen = open(os.path.join(CSRC, "stem_gen.hip")).read()
    dev = open(os.path.join(CSRC, "stem_dev.h")).read()
    assert f"const int m0 = blk * {STEM_TILE};" in gen and f"ceil_div(p.M, {STEM_TILE})" in gen
    assert f"const int grid = ntiles < {STEM_FWD_BLOCKS} ? ntiles : {STEM_FWD_BLOCKS};" in gen
    assert re.search(rf"#define R3M_STEM_WG_BLOCKS {STEM_WG_BLOCKS}\b", dev) and "STEM_WG_BLOCKS = R3M_STEM_WG_BLOCKS" in dev
    assert "total_rows < STEM_WG_BLOCKS ? total_rows : STEM_WG_BLOCKS" in gen


def test_every_condition_is_met_by_a_case():
    assert len(set(STEM_EDGE_CASES)) == len(STEM_EDGE_CASES)
    props = {c: stem_case_props(*c) for c in STEM_EDGE_CASES}
    missing = [name for name, pred in STEM_CONDITIONS.items() if not any(pred(*c, props[c]) for c in STEM_EDGE_CASES)]
    assert not missing, f"no case of STEM_EDGE_CASES meets: {missing}"
    for (F, H, W) in STEM_EDGE_CASES:
        assert 32 <= H <= 512 and 32 <= W <= 512 and F >= 1


# (F, H, W) -> the figures the case was chosen for, as the list's comments state them
NAMED = {
    (1, 32, 32): dict(ntiles=1, straddling=0, last_fill=256, Wo=16),
    (2, 32, 32): dict(ntiles=2, straddling=0, last_fill=256),
    (17, 32, 34): dict(ntiles=19, straddle_phases=list(range(0, 256, 16)), last_fill=16),
    (2, 34, 32): dict(ntiles=3, straddling=1, last_fill=32),
    (3, 33, 35): dict(Wo=18, ntiles=4, straddling=2, last_fill=150),
    (3, 65, 63): dict(Wo=32, m_tiles=1, m_tail=0, lane_trips=1, lane_tail=63),
    (2, 63, 129): dict(Wo=65, m_tiles=3, m_tail=1, lane_trips=3, wo_odd=True),
    (2, 64, 66): dict(Wo=33, m_tiles=2, m_tail=1, lane_trips=2, wo_odd=True),
    (1, 32, 64): dict(Wo=32, lane_trips=1, lane_tail=0),
    (27, 37, 32): dict(wg_rows=513),
    (33, 32, 32): dict(wg_rows=528, straddling=0, ntiles=33),
    (33, 128, 128): dict(ntiles=528, straddling=0),
    (35, 126, 125): dict(ntiles=543, straddling=34, last_fill=163, wg_rows=2205, second_trip_straddles=True),
    (2, 32, 503): dict(Wo=252, straddling=1),
    (2, 37, 512): dict(Wo=256, rows_per_tile_max=2),
    (2, 512, 37): dict(wg_rows=512, dgrad_groups=64),
    (1, 511, 509): dict(Wo=255, invalid_waves=(0, 1)),
}


@pytest.mark.parametrize("case", STEM_EDGE_CASES, ids=lambda c: "F{}_{}x{}".format(*c))
def test_named_figures(case):
    p = stem_case_props(*case)
    for k, v in NAMED[case].items():
        assert p[k] == v, (case, k, p[k], v)


def test_both_loops_take_a_second_trip_with_and_without_straddling_tiles():
    props = [stem_case_props(*c) for c in STEM_EDGE_CASES]
    for cap, key in ((STEM_FWD_BLOCKS, "ntiles"), (STEM_WG_BLOCKS, "wg_rows")):
        assert any(p[key] > cap and p["straddling"] == 0 for p in props), key
        assert any(p[key] > cap and p["straddling"] > 0 for p in props), key
        assert any(p[key] <= cap for p in props), key


def test_the_case_list_reaches_the_largest_lds_footprints():
    """The largest LDS footprint of each of the three kernels over the widths 32..512 (r3m_stem_gen_lds_bytes; tests/test_resolution_plan.py
    bounds it at 160 KiB) is reached by a case: the widest staged row, (2, 37, 512), has the weight gradient's and the input gradient's;
    the forward's (rows of a tile x row stride) is at (2, 32, 503)"""
    from r3m_amd import _lib
    L = _lib.lib()
    f, w, d = C.c_int(), C.c_int(), C.c_int()

    def lds(F, H, W):
        assert L.r3m_stem_gen_lds_bytes(F, H, W, C.byref(f), C.byref(w), C.byref(d)) == 0, L.r3m_last_error()
        return (f.value, w.value, d.value)

    cases = [max(v) for v in zip(*(lds(*c) for c in STEM_EDGE_CASES))]
    sweep = [0, 0, 0]
    for F in (1, 2):
        for H in (32, 37, 64, 255, 512):
            for W in range(32, 513):
                sweep = [max(a, b) for a, b in zip(sweep, lds(F, H, W))]
    assert cases == sweep, (cases, sweep)
    assert lds(2, 37, 512)[1:] == tuple(sweep[1:]) and lds(2, 32, 503)[0] == sweep[0]
    assert [round(v / 1024) for v in lds(2, 37, 512)] == [93, 107, 117], lds(2, 37, 512)
