"""CPU: the conv launch plan (plan_conv, conv.hip) through the host-only scflow_conv_plan_kind —
which kernel family scflow_conv2d launches for an argument struct, which grouped kernel
scflow_conv2d_pair launches for two, and what either answers before launching.  The pointers are
fake 16-byte-aligned integers: nothing is launched or dereferenced.  Without a device device_cus()
is 256, the MI355X's count.

Every expected value was read by hand from the dispatch as it stood BEFORE the plan existed
(commit b92c905: scflow_conv2d at conv.hip:1448-1596, try_pair at conv_pair.h:103-164); the line
each comes from is in the comment beside it."""
import ctypes

import pytest

from scflow_amd import _lib
from scflow_amd._lib import (PAIR_NONE, PAIR_SMALLCIN, PAIR_THIN, PAIR_WINO, PLAN_1X1, PLAN_1X1W,
                             PLAN_MFMA, PLAN_NONE, PLAN_SMALLCIN_GENERIC, PLAN_SMALLCIN_MFMA,
                             PLAN_SMALLCIN_TILED, PLAN_THIN_CHUNKED, PLAN_THIN_FULL,
                             PLAN_THIN_GENERIC, PLAN_THINZ, PLAN_WINO, PLAN_WINO4, PLAN_WINO5)

OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
SRC0, SRC1, WEIGHT, OUT, GATE, RH, HID, WS = (0x10000 * (i + 1) for i in range(8))


def conv(n, h, w, c0, cout, k, bk=16, c1=0, **over):
    """A channels-last conv of kernel k (int: k×k; tuple: kh, kw), "same" padding, dense strides."""
    kh, kw = (k, k) if isinstance(k, int) else k
    a = _lib.ConvArgs()
    a.src0, a.c0, a.s0 = SRC0, c0, c0
    if c1:
        a.src1, a.c1, a.s1 = SRC1, c1, c1
    a.weight, a.out, a.so = WEIGHT, OUT, cout
    a.n, a.h, a.w, a.cout = n, h, w, cout
    a.kh, a.kw, a.ph, a.pw, a.stride = kh, kw, kh // 2, kw // 2, 1
    a.bk = bk
    for key, v in over.items():
        setattr(a, key, v)
    return a


def kind(a, b=None):
    k = ctypes.c_int(-7)
    status = _lib.load().scflow_conv_plan_kind(ctypes.byref(a), ctypes.byref(b) if b is not None else None,
                                               ctypes.byref(k))
    return status, k.value


@pytest.fixture
def switches(monkeypatch):
    def set_(**env):
        for name, v in env.items():
            monkeypatch.setenv(name, str(v))
        _lib.reload_switches()
    yield set_
    monkeypatch.undo()
    _lib.reload_switches()


# the decoder tail's three pairs (scflow_amd/decoder.py: flow predictor ‖ mask predictor, the two
# encoders' first and second layers)
def thin_pair(n, h, w):      # conv_pair.h:112-116
    return conv(n, h, w, 256, 2, 3), conv(n, h, w, 256, 1, 1)


def smallcin_pair(n, h, w):  # conv_pair.h:134-135
    return conv(n, h, w, 2, 128, 7), conv(n, h, w, 1, 64, 3)


def wino_pair(n, h, w):      # conv_pair.h:147, both packed for F(2×2,3×3)
    return conv(n, h, w, 128, 64, 3, _lib.CONV_WINO), conv(n, h, w, 64, 32, 3, _lib.CONV_WINO)


@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("make,expect", [(thin_pair, PAIR_THIN), (smallcin_pair, PAIR_SMALLCIN),
                                         (wino_pair, PAIR_WINO)])
def test_decoder_tail_pairs(make, expect, size):
    # thin: both V_THIN (conv.hip:71-76), a passes thinz_ok (conv.hip:1396-1402: 256 channels, 3×3,
    # pad 1, cout 2, rows % 2 (W=32) / % 4 (W=64) == 0), b is 1×1 → 1, tiled, aligned
    # small-cin: both V_SMALLCIN with mfma_ok (conv_pair.h:59-61), 2/7×7/npad 128 and 1/3×3/npad 64
    # Winograd: wino_nbw (conv.hip:1017-1027) — 128→64: 2·(2·32/4 or 2·64/2 blocks)·1 < 3·256 → 1;
    # 64→32: cout ≤ 32 → 1; both in {1, 2}, one width
    a, b = make(2, size, size)
    assert kind(a, b) == (OK, expect)
    assert kind(b, a) == (OK, expect)  # scflow_conv2d_pair tries both orders (conv.hip:1608-1609)


def test_thin_pair_needs_the_contraction_rows():
    # W = 64, h = 30: thinz_ok wants oh % 4 == 0 (conv.hip:1401) → no pair; each conv is still valid
    # (a runs a tiled LDS kernel: 30 % (64/64) == 0, conv.hip:1542-1543)
    a, b = thin_pair(2, 30, 64)
    assert kind(a, b) == (OK, PAIR_NONE) and kind(b, a) == (OK, PAIR_NONE)
    # W = 32, h = 30: 30 % 2 == 0 satisfies both tiled (64/32 = 2 rows) and thinz_ok, so the pair
    # holds there; an odd height does not tile (conv_pair.h:108-111) → none
    assert kind(*thin_pair(2, 30, 32)) == (OK, PAIR_THIN)
    assert kind(*thin_pair(2, 31, 32)) == (OK, PAIR_NONE)


def test_smallcin_pair_off_under_split(switches):
    switches(SCFLOW_SMALLCIN_SPLIT=1)  # conv_pair.h:62: npad == 128 && smallcin_split() → no plan
    a, b = smallcin_pair(2, 32, 32)
    assert kind(a, b) == (OK, PAIR_NONE) and kind(b, a) == (OK, PAIR_NONE)
    assert kind(a) == (OK, PLAN_SMALLCIN_MFMA)  # still the MFMA kernel, as two workgroups per tile


def test_pairing_off(switches):
    switches(SCFLOW_CONV_PAIR=0)  # conv.hip:1605-1606
    for make in (thin_pair, smallcin_pair, wino_pair):
        assert kind(*make(2, 32, 32)) == (OK, PAIR_NONE)


def test_wino_pair_not_with_96_channel_blocks():
    # 3×3 256→192 at n = 16, 32×32: wino_blocks = 16·(32/4) = 128 (conv.hip:1009), 192 % 96 == 0,
    # 128·(192/96) == 256 CUs and 2·128·3 = 768 is no multiple of 512 → NBW 3 (conv.hip:1023-1025);
    # wino_plan wants 1 or 2 (conv_pair.h:78)
    a = conv(16, 32, 32, 256, 192, 3, _lib.CONV_WINO)
    b = conv(16, 32, 32, 64, 32, 3, _lib.CONV_WINO)
    assert kind(a, b) == (OK, PAIR_NONE) and kind(b, a) == (OK, PAIR_NONE)
    assert kind(a) == (OK, PLAN_WINO)


@pytest.mark.parametrize("make", [thin_pair, smallcin_pair])
def test_mismatched_height_is_no_pair(make):
    a, _ = make(2, 32, 32)  # conv_pair.h:116 / :135: a.h == b.h
    _, b = make(2, 64, 32)
    assert kind(a, b) == (OK, PAIR_NONE) and kind(b, a) == (OK, PAIR_NONE)


@pytest.mark.parametrize("bad", [dict(src0=SRC0 + 4), dict(s0=258)])
def test_pair_with_a_misaligned_half_is_refused(bad):
    # scflow_conv2d answers SCFLOW_EALIGN for this thin conv (conv.hip:1540-1541); the old try_pair
    # did not test a's source (conv_pair.h:112-116) and paired it.  Now the pair is refused before
    # anything is launched, in either order.
    a, b = thin_pair(2, 32, 32)
    for key, v in bad.items():
        setattr(a, key, v)
    assert kind(a) == (EALIGN, PLAN_NONE)
    assert kind(a, b) == (EALIGN, PAIR_NONE)
    assert kind(b, a) == (EALIGN, PAIR_NONE)


def test_bad_packing_format_is_invalid():
    a, b = thin_pair(2, 32, 32)
    a.bk = 5  # conv.hip:1456
    assert kind(a) == (EINVAL, PLAN_NONE)
    assert kind(a, b) == (EINVAL, PAIR_NONE) and kind(b, a) == (EINVAL, PAIR_NONE)
    assert kind(conv(2, 32, 32, 256, 2, 3, out=None)) == (EINVAL, PLAN_NONE)  # conv.hip:1422


GRU = dict(epilogue=_lib.EPI_GRU_ZR, gate=GATE, rh=RH, hid=HID, out=None)
SINGLE = [
    # GRU z|r 1×5 over cat[h, x] → 256, Winograd packing: launch_wino, kh != 3 (conv.hip:1124)
    (conv(16, 32, 32, 128, 256, (1, 5), _lib.CONV_WINO, c1=256, **GRU), {}, PLAN_WINO5),
    (conv(2, 32, 32, 128, 64, 3, _lib.CONV_WINO), {}, PLAN_WINO),  # conv.hip:1136-1146
    # F(4×4,3×3) with a workspace (conv.hip:1453, conv_wino4.h:496-500)
    (conv(2, 32, 32, 128, 512, 3, _lib.CONV_WINO4, ws=WS, ws_bytes=1 << 40), {}, PLAN_WINO4),
    # corr_net.0 324→256, wide 1×1 packing: kb = 41 (conv.hip:1256-1263, 1276-1282)
    (conv(16, 32, 32, 324, 256, 1, _lib.CONV_1X1W), {}, PLAN_1X1W),
    # the same conv from two sources, bk 16: V_MFMA; 16·32·32/128 · 256/64 = 512 workgroups → tile
    # 128 (conv.hip:1153-1159) → conv1x1_kernel (conv.hip:1474-1480); n = 2: 64 < 512 → tile 64 →
    # the direct conv (conv.hip:1483-1487); so does SCFLOW_CONV1X1=0
    (conv(16, 32, 32, 196, 256, 1, c1=60), {}, PLAN_1X1),
    (conv(2, 32, 32, 196, 256, 1, c1=60), {}, PLAN_MFMA),
    (conv(16, 32, 32, 196, 256, 1, c1=60), {"SCFLOW_CONV1X1": 0}, PLAN_MFMA),
    (conv(2, 32, 32, 256, 192, 3), {}, PLAN_MFMA),
    # flow predictor 3×3 256→2: thinz_ok (conv.hip:1550); SCFLOW_THINZ=0: the whole halo fits at
    # W = 32 (4·34 pixels · 260 floats + 18 KiB of weights = 159872 B ≤ 160 KiB, 8704 ≤ 12288
    # float4: conv.hip:1433-1440), at W = 64 it does not (3·66·64 = 12672 float4) → chunked (:1583)
    (conv(2, 32, 32, 256, 2, 3), {}, PLAN_THINZ),
    (conv(2, 32, 32, 256, 2, 3), {"SCFLOW_THINZ": 0}, PLAN_THIN_FULL),
    (conv(2, 64, 64, 256, 2, 3), {"SCFLOW_THINZ": 0}, PLAN_THIN_CHUNKED),
    (conv(2, 32, 32, 256, 2, 3), {"SCFLOW_THINZ": 0, "SCFLOW_THIN_FULL": 0}, PLAN_THIN_CHUNKED),
    (conv(2, 32, 32, 256, 1, 1), {}, PLAN_THIN_CHUNKED),   # mask predictor (conv.hip:1580)
    (conv(2, 32, 32, 128, 3, 3), {}, PLAN_THIN_GENERIC),   # cout 3: in no tiled table (:1588-1594)
    (conv(2, 32, 32, 2, 128, 7), {}, PLAN_SMALLCIN_MFMA),  # conv.hip:1492-1509
    (conv(2, 48, 48, 2, 128, 7), {}, PLAN_SMALLCIN_TILED),  # width 48: no mfma_ok (conv.hip:1516)
    (conv(2, 32, 32, 3, 64, 3), {}, PLAN_SMALLCIN_GENERIC),  # cin 3: in no table (conv.hip:1529-1533)
]


@pytest.mark.parametrize("case", range(len(SINGLE)))
def test_single_kind(case, switches):
    a, env, expect = SINGLE[case]
    switches(**env)
    assert kind(a) == (OK, expect)


def test_single_refusals():
    # width 20 tiles no whole rows: V_NONE (conv.hip:79, 1458)
    assert kind(conv(2, 20, 20, 64, 64, 3)) == (EUNSUPPORTED, PLAN_NONE)
    # F(4×4,3×3) without its workspace (conv_wino4.h:497)
    assert kind(conv(2, 32, 32, 128, 512, 3, _lib.CONV_WINO4)) == (EINVAL, PLAN_NONE)
    # a GRU epilogue on a thin conv (conv.hip:1489)
    assert kind(conv(2, 32, 32, 256, 2, 3, **GRU)) == (EUNSUPPORTED, PLAN_NONE)
    # the direct conv needs an aligned weight pointer (conv.hip:1462-1464)
    assert kind(conv(2, 32, 32, 256, 192, 3, weight=WEIGHT + 8)) == (EALIGN, PLAN_NONE)
    assert _lib.load().scflow_conv_plan_kind(None, None, None) == EINVAL


def test_ops_wrapper():
    from scflow_amd import ops
    a, b = thin_pair(2, 32, 32)
    assert ops.conv_plan_kind(a) == PLAN_THINZ and ops.conv_plan_kind(a, b) == PAIR_THIN
    a.bk = 5
    with pytest.raises(_lib.ScflowError):
        ops.conv_plan_kind(a, b)
