"""CPU: every SCFLOW_* switch of the HIP library is an EnvSwitch, listed in INTEGRATION.md's
"Switches" table, and re-read after reload_switches() — checked through the host-only queries
(no device: device_cus() is 256, as on MI355X).  The expected values are those of the library
before the switches shared one mechanism, run in a fresh process per setting."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scflow_amd", "csrc")


def _csrc():
    return {p: open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*")))}


def _table_rows():
    """name → (where it is read, when it takes effect) of INTEGRATION.md's Switches table."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text.split("## F. Switches", 1)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        m = re.fullmatch(r"`(SCFLOW_[A-Z0-9_]+)`", cells[0])
        if m and line.startswith("|"):
            assert len(cells) == 6, line
            assert m.group(1) not in rows, f"{m.group(1)} listed twice"
            rows[m.group(1)] = (cells[4].strip("`"), cells[5])
    return rows


# ------------------------------------------------------------------------------ completeness
def test_getenv_only_in_envswitch():
    hits = [(os.path.basename(p), i + 1) for p, s in _csrc().items()
            for i, line in enumerate(s.splitlines()) if "getenv(" in line]
    assert len(hits) == 1 and hits[0][0] == "common.h", hits
    common = open(os.path.join(CSRC, "common.h")).read()
    body = common.split("struct EnvSwitch {", 1)[1].split("\n};", 1)[0]
    assert "int get()" in body and "getenv(name)" in body.split("int get()", 1)[1]


def test_table_lists_every_library_switch():
    declared = {}
    for p, s in _csrc().items():
        for name in re.findall(r'EnvSwitch\s+\w+\(\s*"(SCFLOW_[A-Z0-9_]+)"', s):
            assert name not in declared, f"{name} declared in {declared[name]} and {p}"
            declared[name] = os.path.basename(p)
    rows = {n: r for n, r in _table_rows().items() if r[0].startswith("csrc/")}
    assert set(declared) == set(rows)
    for name, f in declared.items():
        assert rows[name][0] == "csrc/" + f, name
        assert rows[name][1].startswith(("every launch", "at pick/pack time")), name


def test_table_lists_every_python_switch():
    rows = _table_rows()
    names = set()
    for p in glob.glob(os.path.join(ROOT, "scflow_amd", "**", "*.py"), recursive=True):
        names |= set(re.findall(r'os\.environ\.get\(\s*"(SCFLOW_[A-Z0-9_]+)"', open(p).read()))
    names -= {"SCFLOW_LIB", "SCFLOW_OFFLOAD_ARCH"}
    assert names, "no Python switch found: the pattern is stale"
    for name in sorted(names):
        assert name in rows, name
        assert rows[name][0].endswith(".py") and rows[name][1] == "at import/construction", name


# ------------------------------------------------------------------------------ reload
@pytest.fixture
def lib():
    from scflow_amd import _lib
    return _lib.load()


def _pick(lib, n, h, w, c0, c1, cout, kh, kw, ph, pw):
    from scflow_amd import _lib
    a = _lib.ConvArgs()
    a.c0, a.c1, a.n, a.h, a.w = c0, c1, n, h, w
    a.cout, a.kh, a.kw, a.ph, a.pw, a.stride = cout, kh, kw, ph, pw, 1
    return lib.scflow_conv_pick_bk(ctypes.byref(a))


def _wgrad_floats(lib, n, h, w, cin, cout, kh, kw, ph, pw):
    from scflow_amd import _lib
    a = _lib.WgradArgs()
    a.n, a.h, a.w, a.cin0, a.cin1, a.cout = n, h, w, cin, 0, cout
    a.kh, a.kw, a.stride, a.ph, a.pw = kh, kw, 1, ph, pw
    a.sdy, a.s0 = cout, cin
    need = ctypes.c_longlong(0)
    assert lib.scflow_conv_wgrad_workspace(ctypes.byref(a), ctypes.byref(need)) == 0
    return need.value


C_256_192 = (16, 32, 32, 256, 0, 192, 3, 3, 1, 1)    # corr_net.1
C_128_64 = (16, 32, 32, 128, 0, 64, 3, 3, 1, 1)
C_1X1 = (16, 32, 32, 324, 0, 256, 1, 1, 0, 0)        # corr_net.0
C_1X1_2SRC = (16, 32, 32, 196, 60, 256, 1, 1, 0, 0)  # two sources: the direct conv
C_256_192_N24 = (24, 32, 32, 256, 0, 192, 3, 3, 1, 1)
DIRECT = {"SCFLOW_CONV_WINO4": "0", "SCFLOW_CONV_WINO": "0"}  # 3×3 convs on the direct kernel
W_3X3 = (2, 32, 32, 64, 64, 3, 3, 1, 1)              # Winograd weight gradient
W_3X3_16 = (2, 16, 16, 64, 64, 3, 3, 1, 1)           # width not a multiple of 32: implicit GEMM
W_1X5 = (2, 32, 32, 64, 64, 1, 5, 0, 2)
W_1X1 = (2, 32, 32, 64, 64, 1, 1, 0, 0)
W_THIN = (2, 32, 32, 256, 2, 3, 3, 1, 1)

# (query, shape, environment, value under it, default)
CASES = [
    (_pick, C_256_192, {"SCFLOW_CONV_WINO4": "0"}, 2, 4),  # the regression guard: was 4 after a reload
    (_pick, C_256_192, DIRECT, 8, 4),
    (_pick, C_256_192, {"SCFLOW_CONV_WINO4": "0", "SCFLOW_CONV_WINO": "5"}, 8, 4),
    (_pick, C_128_64, {"SCFLOW_CONV_WINO4": "2"}, 4, 2),
    (_pick, C_128_64, {"SCFLOW_CONV_WINO": "5"}, 16, 2),
    (_pick, C_128_64, {"SCFLOW_CONV_WINO": "3"}, 2, 2),
    (_pick, C_1X1, {"SCFLOW_CONV1X1W": "0"}, 16, 3),
    (_pick, C_1X1_2SRC, {"SCFLOW_CONV_BK": "8"}, 8, 16),
    (_pick, C_1X1_2SRC, {"SCFLOW_CONV_BK": "16"}, 16, 16),
    (_pick, C_256_192, {**DIRECT, "SCFLOW_CONV_TILE_M": "128"}, 16, 4),      # 8 without TILE_M
    (_pick, C_256_192_N24, {**DIRECT, "SCFLOW_CONV_TILE_M": "64"}, 8, 4),    # 16 without TILE_M
    (_pick, C_256_192_N24, DIRECT, 16, 4),
    (_wgrad_floats, W_3X3, {"SCFLOW_WGRAD_WINO": "0"}, 1181696, 1049600),
    (_wgrad_floats, W_3X3, {"SCFLOW_WGRAD_WINO": "0", "SCFLOW_WGRAD_SPLITS": "1"}, 36928, 1049600),
    (_wgrad_floats, W_3X3, {"SCFLOW_WGRAD_WINO": "0", "SCFLOW_WGRAD_SPLITS": "3"}, 110784, 1049600),
    # the Winograd weight gradient takes this shape first, so the split count alone changes nothing
    (_wgrad_floats, W_3X3, {"SCFLOW_WGRAD_SPLITS": "1"}, 1049600, 1049600),
    (_wgrad_floats, W_3X3_16, {"SCFLOW_WGRAD_SPLITS": "1"}, 36928, 295424),
    (_wgrad_floats, W_3X3_16, {"SCFLOW_WGRAD_SPLITS": "3"}, 110784, 295424),
    (_wgrad_floats, W_1X5, {"SCFLOW_WGRAD_WINO5": "0"}, 657408, 525312),
    (_wgrad_floats, W_1X1, {"SCFLOW_WGRAD_1X1": "0"}, 133120, 8454144),
    (_wgrad_floats, W_THIN, {"SCFLOW_WGRAD_THIN": "0"}, 4720640, 184400),
]


@pytest.mark.parametrize("query,shape,env,value,default", CASES,
                         ids=[f"{c[0].__name__}-{'-'.join(map(str, c[1]))}-" +
                              ",".join(f"{k[7:]}={v}" for k, v in c[2].items()) for c in CASES])
def test_reload_rereads_the_switch(lib, monkeypatch, query, shape, env, value, default):
    from scflow_amd._lib import reload_switches
    reload_switches()
    assert query(lib, *shape) == default
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        assert query(lib, *shape) == default  # cached until the reload
        reload_switches()
        assert query(lib, *shape) == value
    finally:
        for k in env:
            monkeypatch.delenv(k)
        reload_switches()
    assert query(lib, *shape) == default


def test_packed_sizes_follow_the_format_not_a_switch(lib, monkeypatch):
    """scflow_conv_packed_size_bk sizes what scflow_conv_pack_weights writes from the format in
    its arguments alone: no switch moves it between the pick and the pack."""
    from scflow_amd import _lib
    from scflow_amd._lib import reload_switches
    sizes = {_lib.CONV_WINO4: 1769472, _lib.CONV_WINO: 786432, 8: 442368}
    for env in ({}, {"SCFLOW_CONV_WINO4": "0"}, DIRECT, {"SCFLOW_CONV_BK": "8"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        reload_switches()
        try:
            for bk, floats in sizes.items():
                assert lib.scflow_conv_packed_size_bk(192, 256, 0, 3, 3, 1, 32, bk) == floats
        finally:
            for k in env:
                monkeypatch.delenv(k)
            reload_switches()
