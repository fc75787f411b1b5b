"""tests/fullsize_hints.py against the sources it restates: the initialisers of lqcd_internal.h (read from the header text, so the helper cannot drift), make_kargs' map
resolution at 32^3 x 64 and at the smallest shape that resolves like it (32.32.8.4), the volume-adaptive rule of lqcd_ctx_create on the shapes of
tests/test_gpu_fullsize_hints.py, and geometry() of tests/test_cpu_yshare_map.py where both apply."""
import os
import re

import pytest

import fullsize_hints as fh
from test_cpu_yshare_map import geometry

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "latticeqcd.jl_amd", "csrc")
FULL, TWIN = (32, 32, 32, 64), (32, 32, 8, 4)
SMALL_SHAPES = [(16, 8, 8, 4), (32, 8, 8, 4), (16, 16, 16, 8), TWIN]


def test_fullsize_is_the_struct_default():
    text = open(os.path.join(CSRC, "lqcd_internal.h")).read()
    for key, want in fh.FULLSIZE.items():
        m = re.findall(r"^\s*int\s+%s\s*=\s*(-?\d+)\s*;" % key, text, flags=re.M)
        assert len(m) == 1, (key, m)
        assert int(m[0]) == want, (key, m[0], want)
    assert len(re.findall(r"^\s*int\s+nt_active\s*=\s*-1\s*;", text, flags=re.M)) == 1
    assert set(fh.OFF) < set(fh.FULLSIZE) and all(v == 0 for v in fh.OFF.values())


def test_the_adaptive_rule_in_capi_is_the_one_restated():
    text = open(os.path.join(CSRC, "capi.hip")).read()
    assert "slice % 64 == 0 && slice / 64 <= 128) { c->tun.xcd_nsub = 8; c->tun.xcd_ysplit = 2; }" in text
    assert "gauge12_elems(g) * sizeof(double2) <= ((size_t)256 << 20)) c->tun.nt_gauge = 0;" in text
    assert "(size_t)24 * g.Vh * sizeof(double2) <= ((size_t)64 << 20)) c->tun.nt_store = 0;" in text
    assert 'if (!strcmp(key, "nt_active")) return &c->tun.nt_active;' in text


def test_resolve_at_full_size_and_at_its_smallest_twin():
    assert fh.resolve(FULL, 16, 4) == (16, 4, 2, 8, 16, 2)
    assert fh.resolve(TWIN, 16, 4) == (16, 4, 2, 2, 4, 2)
    # the shapes other modules took for that map resolve to something else
    assert fh.resolve((32, 16, 16, 8), 16, 2) == (16, 2, 2, 2, 4, 2)       # (16, 2): two passes, but another split
    assert fh.resolve((16, 16, 16, 4), 16, 4)[1] == 2                       # cpp = 2: the split of 4 falls back to 2
    assert fh.chunks(TWIN) == (64, 8) and 2 * fh.chunks(TWIN)[0] * TWIN[3] == 512      # 512 stencil workgroups, 32768 sites
    assert TWIN[0] * TWIN[1] * TWIN[2] * TWIN[3] == 32768


def test_a_full_size_context_keeps_the_defaults_and_every_small_shape_adapts():
    assert fh.adaptive(FULL) == fh.FULLSIZE
    for L in SMALL_SHAPES + [(8, 4, 6, 2), (6, 6, 4, 2), (8, 4, 6, 4), (16, 8, 8, 8), (8, 8, 8, 16), (8, 4, 6, 8)]:
        a = fh.adaptive(L)
        assert a["nt_gauge"] == 0 and a["nt_store"] == 0, L
    for L in SMALL_SHAPES:
        assert fh.adaptive(L) == fh.ADAPTED, L
    # the thresholds themselves: 32^3 x 16 is the first power-of-two depth whose 12-real links (201 MB) still fit but whose spinor (100 MB) does not
    a = fh.adaptive((32, 32, 32, 16))
    assert (a["nt_gauge"], a["nt_store"], a["xcd_nsub"], a["xcd_ysplit"]) == (0, 1, 16, 4)
    assert fh.adaptive((32, 32, 16, 8))["xcd_nsub"] == 8 and fh.adaptive((32, 32, 18, 8))["xcd_nsub"] == 16      # 128 / 144 chunks per slice


@pytest.mark.parametrize("L2", [8, 16])
@pytest.mark.parametrize("xcd_ysplit", [1, 2])
@pytest.mark.parametrize("L1", [4, 8, 12, 16])
def test_resolve_agrees_with_the_yshare_geometry(L1, xcd_ysplit, L2):
    g = geometry(L1, xcd_ysplit, L2=L2, LT=2)       # its requested nsub is 8 x xcd_ysplit
    nsub, ys, ty, tz, cpr, passes = fh.resolve((32, L1, L2, 2), 8 * xcd_ysplit, xcd_ysplit)
    assert (ys, ty, tz, cpr) == (g["ysplit"], g["ty"], g["tz"], g["cpr"]), (L1, xcd_ysplit, L2)
    assert nsub * cpr == g["cps"] and passes == nsub // 8
