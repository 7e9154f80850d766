"""CPU: the opt-in bf16 3×3 conv (SCFLOW_CONV_BF16_3X3) as far as it goes without a device — the
launch plan through the host-only scflow_conv_plan_kind (fake aligned pointers, nothing launched),
the packed size, the Python knobs and the emulated oracle.  On the parent commit
``_lib.CONV_BF16_3X3`` does not exist and format 7 is SCFLOW_EINVAL."""
import ctypes
import os
import re

import pytest
import torch

from scflow_amd import _lib, ops
from tests import conv3_bf16_restatement as cr
from tests import gru_bf16_restatement as gr

OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
SRC0, SRC1, WEIGHT, OUT, GATE, RH, HID, BMAP = (0x10000 * (i + 1) for i in range(8))
MENC_SHAPES = [(256, 0, 192), (128, 0, 64), (256, 0, 126), (192, 64, 126)]  # (c0, c1, cout)
CASE = (2, 256, 31, 4, 5)  # B, S, input seed, iterations, weight seed (the decoder test's too)


def conv(n, h, w, c0, c1, cout, k=3, bk=None, **over):
    kh, kw = (k, k) if isinstance(k, int) else k
    a = _lib.ConvArgs()
    a.src0, a.c0, a.s0 = SRC0, c0, c0
    if c1:
        a.src1, a.c1, a.s1 = SRC1, c1, c1
    a.weight, a.out, a.so = WEIGHT, OUT, cout
    a.n, a.h, a.w, a.cout = n, h, w, cout
    a.kh, a.kw, a.ph, a.pw, a.stride = kh, kw, kh // 2, kw // 2, 1
    a.gate, a.sg, a.rh, a.srh, a.hid, a.sh = None, 128, None, 128, None, 128
    a.bk = _lib.CONV_BF16_3X3 if bk is None else bk
    for key, v in over.items():
        setattr(a, key, v)
    return a


def kind(a, b=None):
    k = ctypes.c_int(-7)
    status = _lib.load().scflow_conv_plan_kind(ctypes.byref(a), ctypes.byref(b) if b is not None else None,
                                               ctypes.byref(k))
    return status, k.value


def test_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "scflow_hip.h")).read()
    assert int(re.search(r"#define SCFLOW_CONV_BF16_3X3 (\d+)", hdr).group(1)) == _lib.CONV_BF16_3X3 == 7
    assert int(re.search(r"#define SCFLOW_PLAN_C3_BF16 (\d+)", hdr).group(1)) == _lib.PLAN_C3_BF16 == 15
    assert _lib.CONV_BF16 == 6 and _lib.PLAN_SEP_BF16 == 14  # the GRU format keeps its values


# ------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("c0,c1,cout", MENC_SHAPES)
@pytest.mark.parametrize("w", [32, 64])
def test_motion_encoder_shapes_plan_the_bf16_kernel(c0, c1, cout, w):
    planned = (OK, _lib.PLAN_C3_BF16)
    for n in (1, 16):
        assert kind(conv(n, w, w, c0, c1, cout)) == planned
    assert kind(conv(1, 4, w, c0, c1, cout)) == planned  # H = 4: one row block
    a = conv(2, w, w, c0, c1, cout)
    assert _lib.load().scflow_conv_workspace_bytes(ctypes.byref(a)) == 0


def test_any_cout_plans():
    for cout in (1, 2, 31, 33, 127, 129):
        assert kind(conv(2, 8, 32, 64, 0, cout)) == (OK, _lib.PLAN_C3_BF16)


@pytest.mark.parametrize("what,args", [
    ("1×5", conv(2, 32, 32, 128, 128, 128, (1, 5))),
    ("5×5", conv(2, 32, 32, 128, 0, 64, 5)),
    ("stride 2", conv(2, 32, 32, 128, 0, 64, stride=2)),
    ("pad 0", conv(2, 32, 32, 128, 0, 64, ph=0, pw=0)),
    ("W 48", conv(2, 48, 48, 128, 0, 64)),
    ("c0 = 130", conv(2, 32, 32, 130, 0, 64)),
    ("c1 = 16", conv(2, 32, 32, 128, 16, 64)),
    ("GRU z|r epilogue", conv(2, 32, 32, 128, 128, 256, epilogue=_lib.EPI_GRU_ZR, gate=GATE, rh=RH,
                              hid=HID, out=None)),
    ("GRU q epilogue", conv(2, 32, 32, 128, 128, 128, epilogue=_lib.EPI_GRU_Q, gate=GATE, hid=HID,
                            out=None)),
    ("bias map", conv(2, 32, 32, 128, 0, 64, bias_map=BMAP, sbm=64)),
    ("fused input normalisation", conv(2, 32, 32, 128, 0, 64, in_scale=BMAP, in_shift=BMAP)),
    ("fused output normalisation", conv(2, 32, 32, 128, 0, 64, out_scale=BMAP, out_shift=BMAP)),
    ("residual", conv(2, 32, 32, 128, 0, 64, res=BMAP, sres=64)),
    ("H = 6", conv(2, 6, 32, 128, 0, 64)),
    ("sources past 2 GiB of offsets", conv(64, 512, 64, 256, 0, 64)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_outside_the_domain_is_unsupported(what, args):
    assert kind(args) == (EUNSUPPORTED, _lib.PLAN_NONE), what
    assert _lib.load().scflow_conv_workspace_bytes(ctypes.byref(args)) == EUNSUPPORTED, what


def test_alignment_and_argument_checks():
    assert kind(conv(2, 32, 32, 128, 0, 64, s0=386)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 32, 64, s1=34)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 0, 64, src0=SRC0 + 4)) == (EALIGN, _lib.PLAN_NONE)
    assert kind(conv(2, 32, 32, 128, 0, 64, s0=388)) == (OK, _lib.PLAN_C3_BF16)  # any aligned stride
    assert kind(conv(2, 32, 32, 128, 0, 64, out=None)) == (EINVAL, _lib.PLAN_NONE)


def test_the_gru_format_still_refuses_3x3():
    assert kind(conv(2, 32, 32, 128, 128, 128, 3, bk=_lib.CONV_BF16)) == (EUNSUPPORTED, _lib.PLAN_NONE)
    size = _lib.load().scflow_conv_packed_size_bk
    assert size(128, 128, 128, 3, 3, 1, 32, _lib.CONV_BF16) == EUNSUPPORTED
    assert size(128, 128, 128, 1, 5, 1, 32, _lib.CONV_BF16_3X3) == EUNSUPPORTED


def test_a_pair_with_a_bf16_half_is_two_launches():
    a = conv(2, 32, 32, 256, 0, 192)
    for b in (conv(2, 32, 32, 128, 0, 64),                                # bf16 beside bf16
              conv(2, 32, 32, 128, 0, 64, 3, bk=_lib.CONV_WINO),          # beside F(2×2,3×3)
              conv(2, 32, 32, 128, 128, 128, (1, 5), bk=_lib.CONV_BF16),  # beside the GRU's bf16 conv
              conv(2, 32, 32, 256, 0, 1, 1, bk=16)):                      # beside a thin conv
        assert kind(a, b) == (OK, _lib.PAIR_NONE) and kind(b, a) == (OK, _lib.PAIR_NONE)
    bad = conv(2, 32, 32, 130, 0, 64)
    assert kind(a, bad) == (EUNSUPPORTED, _lib.PAIR_NONE)


def test_packed_size_is_the_headers_formula():
    size = _lib.load().scflow_conv_packed_size_bk
    for c0, c1, cout in MENC_SHAPES + [(32, 0, 33), (32, 0, 32), (64, 32, 1)]:
        for w in (32, 64):
            want = (cout + 31) // 32 * 32 * (c0 + c1) * 9 // 2  # two bf16 per float, cout padded to 32
            assert size(cout, c0, c1, 3, 3, 1, w, _lib.CONV_BF16_3X3) == want
    assert size(64, 128, 0, 5, 5, 1, 32, _lib.CONV_BF16_3X3) == EUNSUPPORTED
    assert size(64, 128, 0, 3, 3, 2, 32, _lib.CONV_BF16_3X3) == EUNSUPPORTED
    assert size(64, 130, 0, 3, 3, 1, 32, _lib.CONV_BF16_3X3) == EUNSUPPORTED
    assert size(64, 128, 16, 3, 3, 1, 32, _lib.CONV_BF16_3X3) == EUNSUPPORTED
    assert size(64, 128, 0, 3, 3, 1, 48, _lib.CONV_BF16_3X3) == EUNSUPPORTED
    assert size(64, 128, 0, 3, 3, 1, 32, 5) == EINVAL  # 5 stays no format


def test_pick_bk_never_returns_the_format():
    for c0, c1, cout in MENC_SHAPES + [(64, 0, 32), (32, 0, 33)]:
        for n, s in ((1, 32), (2, 32), (16, 32), (1, 64), (32, 64)):
            bk = ops.conv_pick_bk(n, s, s, c0, c1, cout, 3, 3, 1, 1)
            assert bk in (8, 16, _lib.CONV_WINO, _lib.CONV_WINO4), (c0, c1, cout, n, s, bk)
    assert ops.conv_pick_bk(1, 4, 32, 256, 0, 192, 3, 3, 1, 1) != _lib.CONV_BF16_3X3


# ------------------------------------------------------------------------------------- the knobs
def test_motion_encoder_flag_picks_the_three_runners_format():
    from scflow_amd.modules import ConvRunner, MotionEncoder
    enc = MotionEncoder(act_cfg=dict(type="ReLU"))
    assert enc.bf16 is False

    def fmt(m):
        return ConvRunner.of(m.conv, m.act_type).fmt
    wired = [enc.corr_net[1], enc.flow_net[1], enc.out_net[0]]
    assert [m.conv.kernel_size for m in wired] == [(3, 3)] * 3
    assert [r.fmt for r in enc.runners()] == [None] * 3
    enc.bf16 = True
    assert [r.fmt for r in enc.runners()] == [_lib.CONV_BF16_3X3] * 3
    assert [fmt(m) for m in wired] == [_lib.CONV_BF16_3X3] * 3
    assert fmt(enc.corr_net[0]) is None and fmt(enc.flow_net[0]) is None  # the 1×1 and the 7×7
    enc.bf16 = False
    assert [r.fmt for r in enc.runners()] == [None] * 3
    assert [fmt(m) for m in wired] == [None] * 3
    assert fmt(enc.corr_net[0]) is None and fmt(enc.flow_net[0]) is None


def test_a_runner_with_the_format_does_not_ask_the_library(monkeypatch):
    from scflow_amd.modules import ConvRunner
    r = ConvRunner([torch.nn.Conv2d(128, 64, 3, padding=1)], "ReLU")
    plain = r._pick(2, 32, 32, 128, 0)
    assert plain != _lib.CONV_BF16_3X3
    r.fmt = _lib.CONV_BF16_3X3
    monkeypatch.setattr(ops, "conv_pick_bk", lambda *a, **k: pytest.fail("asked the library"))
    assert r._pick(2, 32, 32, 128, 0) == _lib.CONV_BF16_3X3
    r._bk = _lib.CONV_BF16_3X3
    assert r.mfma_flops(2048, 128) == 2.0 * 2048 * 64 * 9 * 128
    monkeypatch.undo()
    r.fmt = None
    assert r._pick(2, 32, 32, 128, 0) == plain


def test_decoders_default_to_fp32():
    from scflow_amd.recurrent import _RecurrentDecoder
    from tests import raft_restatement as rr
    from tests.test_gpu_decoder import build_decoder
    for dec in (build_decoder(2), rr.build_raft_decoder("RAFTDecoder", 2),
                rr.build_raft_decoder("RAFTDecoderMask", 2)):
        assert isinstance(dec, _RecurrentDecoder)
        assert dec.menc_bf16 is False and dec.encoder.bf16 is False and dec.gru_bf16 is False


def test_training_never_selects_the_format():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scflow_amd",
                            "train", "model.py")).read()
    assert "BF16" not in src and "menc_bf16" not in src


# ------------------------------------------------------------------------------------- the oracle
def test_emulated_oracle_is_finite_and_differs_from_fp32():
    """The decoder test's yardstick at its shape (B = 2, 256², 4 iterations, synthetic weights):
    D_ref > 0 for every output family — the rounding moves every output the test looks at."""
    _, _, ref, emu = cr.oracle_pair(*CASE)
    for lst in emu:
        assert all(torch.isfinite(v).all() for v in lst)
    d = gr.distances(emu, ref)
    print("D_ref", d)
    assert all(0 < d[f] < float("inf") for f in gr.FAMILIES), d


def test_emulation_rounds_only_the_three_3x3_convs():
    """With bf16-representable weights and activations that stay representable the emulation is
    the oracle's motion_encoder bit for bit; it ignores sub-bf16 changes of the three 3×3 convs'
    weights and sees them in corr_net.0's and flow_net.0's."""
    from oracle import scflow_oracle as orc
    g = torch.Generator().manual_seed(7)
    shapes = {"corr_net.0": (8, 12, 1, 1), "corr_net.1": (8, 8, 3, 3), "flow_net.0": (8, 2, 7, 7),
              "flow_net.1": (8, 8, 3, 3), "out_net.0": (6, 16, 3, 3)}
    sd = {f"encoder.{k}.conv.weight": cr.round_bf16(torch.randn(s, generator=g) * 0.2)
          for k, s in shapes.items()}
    sd.update({f"encoder.{k}.conv.bias": torch.randn(s[0], generator=g) * 0.1 for k, s in shapes.items()})
    corr = torch.randn(1, 12, 8, 8, generator=g)
    flow = torch.randn(1, 2, 8, 8, generator=g)
    a, b = orc.motion_encoder(sd, corr, flow), cr.motion_encoder_bf16(sd, corr, flow)
    assert a.shape == b.shape == (1, 8, 8, 8)
    assert not torch.equal(a, b)                 # the activations are rounded
    assert torch.equal(a[:, 6:], b[:, 6:])       # the appended flow channels are not
    tiny = 1 + 2 ** -13  # a 16th of a bf16 half-ulp: rounded away where the emulation rounds

    def scaled(key):
        out = dict(sd)
        out[f"encoder.{key}.conv.weight"] = sd[f"encoder.{key}.conv.weight"] * tiny
        return out
    for key in ("corr_net.1", "flow_net.1", "out_net.0"):
        assert torch.equal(cr.motion_encoder_bf16(scaled(key), corr, flow), b), key
        assert not torch.equal(orc.motion_encoder(scaled(key), corr, flow), a), key
    for key in ("corr_net.0", "flow_net.0"):
        assert not torch.equal(cr.motion_encoder_bf16(scaled(key), corr, flow), b), key


def test_the_emulation_is_removed_again():
    from oracle import scflow_oracle as orc
    plain = orc.motion_encoder, orc.conv_gru
    with cr.emulating(128):
        assert orc.motion_encoder is cr.motion_encoder_bf16 and orc.conv_gru is not plain[1]
    assert (orc.motion_encoder, orc.conv_gru) == plain
    with pytest.raises(RuntimeError):
        with cr.emulating():
            assert orc.conv_gru is plain[1]
            raise RuntimeError("inside")
    assert (orc.motion_encoder, orc.conv_gru) == plain
