"""CPU: the weight-gradient launch plan (plan_wgrad, train.hip) through the host-only
scflow_conv_wgrad_plan — which kernel family scflow_conv_wgrad / _batched launch for an argument
struct, how many workspace floats that launch needs, and what either answers before launching.
The pointers are fake 16-byte-aligned integers: nothing is launched or dereferenced.  Without a
device device_cus() is 256, the MI355X's count.

Every expected kind was read by hand from the three if-chains as they stood BEFORE the plan
existed (commit 676e954: scflow_conv_wgrad_workspace at train.hip:1808-1836, _batched at
1905-1951, scflow_conv_wgrad at 1953-1985) and the geometry functions they call (wthin_geometry
train.hip:731-769, wwino_geometry wgrad_wino.h:446-473, wwino5_geometry wgrad_wino5.h:376-409,
w1_geometry wgrad_1x1.h:159-196, wgrad_geometry train.hip:653-707); the line each comes from is
in the comment beside it.  The query floats are what 676e954's library answered for
scflow_conv_wgrad_workspace on a machine without a device."""
import ctypes

import pytest

from scflow_amd import _lib
from scflow_amd._lib import WGRAD_1X1, WGRAD_GEMM, WGRAD_NONE, WGRAD_THIN, WGRAD_WINO, WGRAD_WINO5

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
DY, SRC0, SRC1, DW, DB, WS = (0x10000 * (i + 1) for i in range(6))


def walk(n, h, w, cin0, cout, k, stride=1, cin1=0, pad=None):
    """The walk of a channels-last conv of kernel k (int: k×k; tuple: kh, kw), padding k // 2
    unless given, dense strides, n images in all."""
    kh, kw = (k, k) if isinstance(k, int) else k
    a = _lib.WgradArgs()
    a.dy, a.sdy = DY, cout
    a.src0, a.cin0, a.s0 = SRC0, cin0, cin0
    if cin1:
        a.src1, a.cin1, a.s1 = SRC1, cin1, cin1
    a.dw, a.db, a.workspace, a.workspace_floats = DW, DB, WS, 1 << 40
    a.n, a.h, a.w, a.cout, a.kh, a.kw, a.stride = n, h, w, cout, kh, kw, stride
    a.ph, a.pw = (kh // 2, kw // 2) if pad is None else pad
    return a


def with_(a, **over):
    for key, v in over.items():
        setattr(a, key, v)
    return a


def plan(a, segs):
    kind, floats = ctypes.c_int(-7), ctypes.c_longlong(-7)
    status = _lib.load().scflow_conv_wgrad_plan(ctypes.byref(a), segs, ctypes.byref(kind),
                                                ctypes.byref(floats))
    return status, kind.value, floats.value


def query(a):
    floats = ctypes.c_longlong(-7)
    return _lib.load().scflow_conv_wgrad_workspace(ctypes.byref(a), ctypes.byref(floats)), floats.value


@pytest.fixture
def switches(monkeypatch):
    def set_(**env):
        for name, v in env.items():
            monkeypatch.setenv(name, str(v))
        _lib.reload_switches()
    yield set_
    monkeypatch.undo()
    _lib.reload_switches()


# (name, walk, kind, the floats 676e954's scflow_conv_wgrad_workspace answers)
CASES = [
    # Winograd 3×3: thin refuses (cout and cin > 4, train.hip:740-745); 3×3 stride 1 pad 1,
    # h % 4 == 0, w % 32 == 0, float4 channel groups, cout ≥ 64, cin ≥ 16 (wgrad_wino.h:450-455)
    ("wino 128→64 16×32²", walk(16, 32, 32, 128, 64, 3), WGRAD_WINO, 8392704),
    ("wino 64⊕32→96 6×32×64", walk(6, 32, 64, 64, 96, 3, cin1=32), WGRAD_WINO, 6294528),
    # F(4,5): not 3×3 (wgrad_wino.h:450); 1×5 pad (0, 2) / 5×1 pad (2, 0), the walked image
    # H % 4 == 0 and W % 32 == 0, cout ≥ 64 (wgrad_wino5.h:381-392)
    ("wino5 1×5 128⊕128→256", walk(16, 32, 32, 128, 256, (1, 5), cin1=128), WGRAD_WINO5, 8392704),
    ("wino5 5×1 128⊕128→128", walk(16, 32, 32, 128, 128, (5, 1), cin1=128), WGRAD_WINO5, 8392704),
    # thin: cout ≤ 4 with float4 input channels ≤ 256 (train.hip:740-742), or cin ≤ 4 from one
    # source with float4 output channels ≤ 256 (743-744); kw in {1, 3, 5}, kh ≤ 5, stride ≤ 2 (738-739)
    ("thin 3×3 256→2", walk(16, 32, 32, 256, 2, 3), WGRAD_THIN, 1217040),
    ("thin 1×1 256→1", walk(16, 32, 32, 256, 1, 1), WGRAD_THIN, 67848),
    ("thin 3×3 1→64", walk(16, 32, 32, 1, 64, 3), WGRAD_THIN, 168960),
    ("thin 5×5/2 2→64 5×20×24", walk(5, 20, 24, 2, 64, 5, stride=2), WGRAD_THIN, 58752),
    # 1×1: thin refuses (both sides > 4), not 3×3, not 1×5 / 5×1; 1×1 pad 0 stride 1 or 2,
    # float4 channel groups, any image size (wgrad_1x1.h:162-169)
    ("1x1 324→256", walk(16, 32, 32, 324, 256, 1), WGRAD_1X1, 8377600),
    ("1x1 /2 64→96 2×33×31", walk(2, 33, 31, 64, 96, 1, stride=2), WGRAD_1X1, 8454144),
    # implicit GEMM: stride 2 (wgrad_wino.h:450), w % 32 != 0 (:451) and cout < 64 (:455) each
    # refuse Winograd; wgrad_geometry tiles them (train.hip:662-670: /2 at 64² → 32² outputs,
    # tc 16 tr 2; 16² → tc 16 tr 4; 32² → tc 32 tr 2)
    ("gemm 3×3/2 64→128 16×64²", walk(16, 64, 64, 64, 128, 3, stride=2), WGRAD_GEMM, 7607168),
    ("gemm 3×3 64→64 2×16²", walk(2, 16, 16, 64, 64, 3), WGRAD_GEMM, 295424),
    ("gemm 3×3 64→64 2×8²", walk(2, 8, 8, 64, 64, 3), WGRAD_GEMM, 73856),
    ("gemm 3×3 64→32 2×32²", walk(2, 32, 32, 64, 32, 3), WGRAD_GEMM, 1181696),
]
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("name,a,kind,floats", CASES, ids=IDS)
def test_kind_and_query_floats(name, a, kind, floats):
    assert query(a) == (OK, floats)
    assert plan(a, 0) == (OK, kind, floats)
    # the query answers for null pointers too (tests/test_switches.py calls it that way)
    for key in ("dy", "src0", "src1", "dw", "db", "workspace"):
        setattr(a, key, None)
    a.workspace_floats = 0
    try:
        assert query(a) == (OK, floats) and plan(a, 0) == (OK, kind, floats)
    finally:
        a.dy, a.src0, a.dw, a.db, a.workspace, a.workspace_floats = DY, SRC0, DW, DB, WS, 1 << 40
        a.src1 = SRC1 if a.cin1 else None


@pytest.mark.parametrize("name,a,kind,floats", CASES, ids=IDS)
def test_launch_need_is_within_the_query(name, a, kind, floats):
    """What a launch over segs segments needs never exceeds what the query sized for any segment
    count: otherwise scflow_conv_wgrad_batched answers SCFLOW_EINVAL and functions._flush_wgrad_same
    silently runs one launch per use."""
    a.workspace_floats = floats  # as ops allocates it
    try:
        for segs in range(1, 9):
            if a.n % segs:
                continue
            status, k, need = plan(a, segs)
            assert (status, k) == (OK, kind), segs
            assert 0 < need <= floats, segs
    finally:
        a.workspace_floats = 1 << 40


def test_thin_launch_floats():
    # 5×5/2 2→64, 24 × 20×24: 10×12 outputs (train.hip:748-749), pix = 2880, ppb = max(64,
    # ⌈2880/512⌉) = 64 (759-761); rows = segs·⌈nimg·120/64⌉ (765-766): 1·45, 3·15, 8·⌈360/64⌉ = 8·6;
    # the query: 45 + 8 (767); a row holds cout·cin·kh·kw + cout = 64·2·25 + 64 = 3264 floats (908)
    a = walk(24, 20, 24, 2, 64, 5, stride=2)
    assert [plan(a, s) for s in (0, 1, 3, 8)] == [(OK, WGRAD_THIN, r * 3264) for r in (53, 45, 45, 48)]


def test_1x1_launch_floats():
    # 324→256, 24 × 32²: tiles = 2·3, want = min(⌈512/6⌉ = 86, 8 Mi / (256·384) = 85) = 85
    # (wgrad_1x1.h:181-185), the query max(85, 8) splits (187); a launch: spl = ⌊85/segs⌋ capped by
    # ⌈seg_pix/64⌉, pps = ⌈seg_pix/spl⌉ rounded up to 16, spl = ⌈seg_pix/pps⌉ (188-194):
    #   segs 1: 85 → pps 290 → 304 → 81;  3: 28 → 293 → 304 → 27 (81 in all);  8: 10 → 308 → 320 → 10
    # a split holds copad·cinp + copad = 256·384 + 256 = 98560 floats (200, 206)
    a = walk(24, 32, 32, 324, 256, 1)
    assert [plan(a, s) for s in (0, 1, 3, 8)] == [(OK, WGRAD_1X1, r * 98560) for r in (85, 81, 81, 80)]


REFUSED = [
    # 7×7: thin takes kw in {1, 3, 5} (train.hip:738), wgrad_geometry 1×1 / 3×3 / 1×5 / 5×1 (655-657)
    walk(16, 32, 32, 2, 128, 7),
    # 3×3 at 30×30: w % 32 (wgrad_wino.h:451); tc = 30 is no power of two (train.hip:664)
    walk(2, 30, 30, 64, 64, 3),
    walk(2, 32, 32, 64, 64, 5),             # 5×5 with both sides > 4: train.hip:745, 655-657
    walk(2, 32, 32, 64, 64, 1, pad=(1, 1)),  # wgrad_1x1.h:162; 34 outputs per row: train.hip:664
    # 1×5 without its padding: wgrad_wino5.h:381-386; 28 outputs per row: train.hip:664
    walk(2, 32, 32, 128, 128, (1, 5), pad=(0, 0)),
]


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_refused(case):
    a = REFUSED[case]
    assert query(a)[0] == EUNSUPPORTED
    for segs in (0, 1, 2):
        assert plan(a, segs) == (EUNSUPPORTED, WGRAD_NONE, 0)


@pytest.mark.parametrize("switch,a", [
    ("SCFLOW_WGRAD_THIN", walk(16, 32, 32, 256, 2, 3)),    # train.hip:732-733
    ("SCFLOW_WGRAD_THIN", walk(16, 32, 32, 256, 1, 1)),    # 1×1 wants cout > 4 (wgrad_1x1.h:166)
    ("SCFLOW_WGRAD_WINO", walk(16, 32, 32, 128, 64, 3)),   # wgrad_wino.h:447-448
    ("SCFLOW_WGRAD_WINO5", walk(16, 32, 32, 128, 256, (1, 5), cin1=128)),  # wgrad_wino5.h:377-378
    ("SCFLOW_WGRAD_1X1", walk(16, 32, 32, 324, 256, 1)),   # wgrad_1x1.h:160-161
])
def test_switch_sends_the_shape_to_the_implicit_gemm(switch, a, switches):
    """Each special family switched off hands its shape to the next family that takes it: the
    other three special families are disjoint from it, so that is the implicit GEMM."""
    assert plan(a, 1)[:2] != (OK, WGRAD_GEMM)
    switches(**{switch: 0})
    for segs in (0, 1, 2, 8):
        status, kind, floats = plan(a, segs)
        assert (status, kind) == (OK, WGRAD_GEMM) and floats == query(a)[1]


def test_argument_check():
    lib = _lib.load()
    good = lambda **over: with_(walk(16, 32, 32, 128, 64, 3), **over)  # noqa: E731
    for bad in (good(n=0), good(sdy=60), good(s0=124), good(cin1=32, s1=16, src1=SRC1), good(ph=-1)):
        assert query(bad)[0] == EINVAL
        for segs in (0, 1, 2):
            assert plan(bad, segs) == (EINVAL, WGRAD_NONE, 0)
    two = good(cin1=32, s1=32)  # a second source without its pointer: fine to size, not to launch
    assert plan(two, 0)[:2] == (OK, WGRAD_WINO) and plan(two, 1) == (EINVAL, WGRAD_NONE, 0)
    for key in ("dy", "src0", "dw", "workspace"):
        assert plan(good(**{key: None}), 0)[0] == OK and plan(good(**{key: None}), 1)[0] == EINVAL
    assert plan(good(db=None), 1)[:2] == (OK, WGRAD_WINO)  # the bias gradient is optional
    assert plan(good(), 9)[0] == EINVAL and plan(good(), -1)[0] == EINVAL
    assert plan(good(), 3)[0] == EINVAL  # 16 images are not three equal segments
    # a workspace smaller than the launch needs: refused, with the need reported
    assert plan(good(workspace_floats=8392703), 2) == (EINVAL, WGRAD_WINO, 8392704)
    a, k, f = good(), ctypes.c_int(0), ctypes.c_longlong(0)
    assert lib.scflow_conv_wgrad_plan(None, 1, ctypes.byref(k), ctypes.byref(f)) == EINVAL
    assert lib.scflow_conv_wgrad_plan(ctypes.byref(a), 1, None, ctypes.byref(f)) == EINVAL
    assert lib.scflow_conv_wgrad_plan(ctypes.byref(a), 1, ctypes.byref(k), None) == EINVAL


def test_the_launches_refuse_what_the_plan_refuses():
    """scflow_conv_wgrad_batched applies the single call's shape check (it used to test only the
    pointers), and both return before anything is launched."""
    lib = _lib.load()
    arr = ctypes.c_void_p * 2
    dys, s0s = arr(DY, DY + 0x1000), arr(SRC0, SRC0 + 0x1000)
    for bad in (dict(sdy=60), dict(s0=124), dict(h=0), dict(pw=-1), dict(n=0), dict(workspace_floats=16)):
        a = with_(walk(8, 32, 32, 128, 64, 3), **bad)
        assert lib.scflow_conv_wgrad_batched(ctypes.byref(a), 2, dys, s0s, None, None) == EINVAL
        assert lib.scflow_conv_wgrad(ctypes.byref(a), None) == EINVAL
    a = walk(8, 30, 30, 64, 64, 3)
    assert lib.scflow_conv_wgrad_batched(ctypes.byref(a), 2, dys, s0s, None, None) == EUNSUPPORTED
    assert lib.scflow_conv_wgrad(ctypes.byref(a), None) == EUNSUPPORTED
    a = walk(8, 32, 32, 128, 64, 3)
    assert lib.scflow_conv_wgrad_batched(ctypes.byref(a), 2, arr(DY, DY + 4), s0s, None, None) == EINVAL
    assert lib.scflow_conv_wgrad_batched(ctypes.byref(a), 2, arr(DY, None), s0s, None, None) == EINVAL
    assert lib.scflow_conv_wgrad_batched(ctypes.byref(a), 9, dys, s0s, None, None) == EINVAL
